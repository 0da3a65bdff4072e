"""Generate tests/golden/wct_np_mix_reference.npz by EXECUTING the reference's own `wct_np` (ops.py:92-140).

    python tools/make_mix_golden.py          (needs the reference tree: WCT_REFERENCE, default as in oracle/make_golden.py)

A style mix is sum_k lambda_k wct_np(content, style_k, alpha) (Li et al. 2017, sec. 4.2).  The fixture keeps the reference's
output for every style on its own; the tests form the weighted sums.  One seeded content and three seeded styles of
different sizes per channel count, rebuilt from their seeds by synthetic_features_exact (identical on every host); every
style has more pixels than channels, so no kept count sits on the reference's 1e-5 cut-off.  For C = 256 the fixture keeps
N_ROWS seeded content rows of each output (the file stays well under 1 MB); for C = 64 all of them.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.make_golden import REF, lift_function  # noqa: E402
from wct_tf_amd.weights import synthetic_features_exact  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'wct_np_mix_reference.npz')
ALPHA = 0.8
N_ROWS = 96
# name, C, content (seed, h, w), styles [(seed, h, w)] x 3
CASES = [
    ('c64', 64, (8101, 16, 16), [(8201, 12, 20), (8202, 16, 16), (8203, 10, 14)]),
    ('c256', 256, (8102, 17, 16), [(8204, 18, 16), (8205, 20, 16), (8206, 17, 17)]),
]


def case_inputs(case):
    """(content [1][h][w][C], [style [1][h][w][C]] x 3) of a case, rebuilt from the seeds"""
    name, c, (sc, hc, wc), styles = case
    return (synthetic_features_exact(sc, c, hc, wc, 2.0),
            [synthetic_features_exact(s, c, h, w, 2.0) for s, h, w in styles])


def case_rows(case):
    """the content rows the fixture keeps (all of them for C = 64)"""
    name, c, (sc, hc, wc), _ = case
    if c == 64:
        return np.arange(hc * wc)
    return np.sort(np.random.default_rng(sc).choice(hc * wc, N_ROWS, replace=False))


def main():
    ref_wct_np = lift_function(os.path.join(REF, 'ops.py'), 'wct_np')
    blob = {'alpha': np.float64(ALPHA)}
    for case in CASES:
        name, c = case[:2]
        fc, styles = case_inputs(case)
        rows = case_rows(case)
        blob[name + '/rows'] = rows
        for k, fs in enumerate(styles):
            out = ref_wct_np(fc, fs, ALPHA)
            assert out.dtype == np.float32 and out.shape == fc.shape
            blob['%s/out%d' % (name, k)] = out.reshape(-1, c)[rows]
    np.savez_compressed(OUT, **blob)
    print(OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
