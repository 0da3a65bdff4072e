"""Cost of --content-size on a video that arrives larger: the resize on a host core (Pillow, today's route) against the resize on
the device (resize=, what stylize_video --device-resize does), end to end and in one process.

    python tools/bench_resize_video.py [--rounds R] [--out profiles/resize_video_bench.json]

64 synthetic frames of 1080 x 1920 in host memory (no image decoding), --content-size 512 (512 x 910), five levels, one prepared
style, alpha 0.8, at batch 8 and batch 32.  Two routes over the same frames, host frames in to host frames out:
  host     utils.resize_to on every frame (Pillow, one core), then predict_frames on the resized frames
  device   predict_frames(raw frames, resize=(512, 910)): the raw frames go up, are resized there, and are stylized
The host resize is inside the clock: it is the point.  Each route is measured in R rounds of one pass over the video (a host
clock around calls that end in a device synchronise); the routes alternate within a round.  Per batch size: the median ms per
frame of each, host / device, and the spread of each route's rounds, (max - min) / median -- the margin a difference has to
exceed.  The frames of the two routes are checked once (they must be equal).  Also the op alone: wct_resize_batch_dev at
B = 32 on frames resident in HBM, a host clock around 20 launches and one synchronise, and Pillow alone per frame.  Nothing is
gated on the numbers.  Writes one JSON file and prints it.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from wct_tf_amd import utils  # noqa: E402
from wct_tf_amd.wct import WCT  # noqa: E402
from wct_tf_amd.weights import RELU_TARGETS, synthetic_image, synthetic_weights  # noqa: E402

RAW = (1080, 1920)
SHORT = 512
FRAMES = 64
OP_LAUNCHES = 20


def timed_ms(fn):
    t0 = time.perf_counter()
    fn()                                       # blocking: every call inside ends in a device synchronise
    return (time.perf_counter() - t0) * 1e3


def synthetic_video(n, h, w):
    """n frames of smooth structure plus noise: a coarse random field upscaled, so that neighbouring pixels are correlated as
    in footage, with a random byte of grain"""
    rng = np.random.RandomState(7)
    out = np.empty((n, h, w, 3), np.uint8)
    for i in range(n):
        coarse = rng.randint(0, 256, (h // 40 + 1, w // 40 + 1, 3)).astype(np.uint8)
        base = utils._imresize(coarse, (h, w)).astype(np.int16)
        out[i] = np.clip(base + rng.randint(-16, 17, (h, w, 3)), 0, 255)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'resize_video_bench.json'))
    args = ap.parse_args()
    rounds = max(3, args.rounds)
    model = WCT(None, RELU_TARGETS, None, weights=synthetic_weights(42))
    ctx = model.sess
    video = synthetic_video(FRAMES, *RAW)
    size = utils.resize_shape(RAW[0], RAW[1], SHORT)
    handle = model.prepare_style(synthetic_image(2000, 512, 512))

    def host(batch):
        return model.predict_frames(np.stack([utils.resize_to(f, SHORT) for f in video]), handle, alpha=0.8, batch=batch)

    def device(batch):
        return model.predict_frames(video, handle, alpha=0.8, batch=batch, resize=size)

    res = {'raw_frame': list(RAW), 'content_size': SHORT, 'frame': list(size), 'levels': len(RELU_TARGETS), 'alpha': 0.8,
           'rounds': rounds, 'video_frames': FRAMES,
           'unit': 'ms per frame, host clock around blocking calls over all %d frames, host frames in to host frames out' % FRAMES,
           'cases': {}}
    for batch in (8, 32):
        routes = {'host': lambda: host(batch), 'device': lambda: device(batch)}
        same = bool(np.array_equal(routes['host'](), routes['device']()))        # also the warm-up of both
        ms = {k: [] for k in routes}
        for _ in range(rounds):
            for k, fn in routes.items():
                ms[k].append(timed_ms(fn) / FRAMES)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        res['cases']['video64_batch%d' % batch] = {
            'host_ms_per_frame': round(med['host'], 4), 'device_ms_per_frame': round(med['device'], 4),
            'host_over_device': round(med['host'] / med['device'], 4),
            'host_spread': round((max(ms['host']) - min(ms['host'])) / med['host'], 4),
            'device_spread': round((max(ms['device']) - min(ms['device'])) / med['device'], 4),
            'frames_equal': same}
        print(batch, res['cases']['video64_batch%d' % batch], flush=True)

    # the op alone, B = 32 resident in HBM; and Pillow alone
    b = 32
    src, dst = ctx.dev_alloc(video[:b].nbytes), ctx.dev_alloc(b * size[0] * size[1] * 3)
    try:
        ctx.h2d(src, video[:b])

        def op():
            for _ in range(OP_LAUNCHES):
                ctx.resize_batch_dev(src, RAW[0], RAW[1], b, size, dst)
            ctx.sync()

        op()
        op_ms = [timed_ms(op) / OP_LAUNCHES for _ in range(rounds)]
        got = np.empty((b,) + size + (3,), np.uint8)
        ctx.d2h(got, dst)
    finally:
        ctx.dev_free(src)
        ctx.dev_free(dst)
    pil_ms = [timed_ms(lambda: [utils.resize_to(f, SHORT) for f in video[:8]]) / 8 for _ in range(rounds)]
    res['op_alone'] = {
        'batch': b, 'launch_ms': round(float(np.median(op_ms)), 4), 'ms_per_frame': round(float(np.median(op_ms)) / b, 5),
        'spread': round((max(op_ms) - min(op_ms)) / float(np.median(op_ms)), 4),
        'gbytes_per_s_in_plus_out': round((video[:b].nbytes + got.nbytes) / (float(np.median(op_ms)) * 1e-3) / 1e9, 1),
        'pillow_ms_per_frame_one_core': round(float(np.median(pil_ms)), 3),
        'equals_pillow': bool(np.array_equal(got, np.stack([utils.resize_to(f, SHORT) for f in video[:b]])))}
    print(res['op_alone'], flush=True)
    handle.close()
    ctx.close()
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
