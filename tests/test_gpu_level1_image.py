"""relu1_1 computed where it is read: wct_stylize_batch_dev takes the level-1 covariance of both sides and the
apply's content rows from the images (cov_image_kernel, apply_image_kernel) and stores no fp32 relu1_1 -- the conv1_1 passes
take the unit sums alone (the style's beside the fp16 map conv1_2 reads).  The frames must be the ones of the stored-feature
path, bit for bit: the reference is this library in a fresh child process with WCT_L1_FROM_IMAGE=0 (the switch is read once per
process), which runs the same cases through the same code below."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

L1 = ['relu1_1']
L21 = ['relu2_1', 'relu1_1']
L5 = ['relu5_1', 'relu4_1', 'relu3_1', 'relu2_1', 'relu1_1']

# name: (content key, style key, levels, alpha, wct_mode).  Content 40x80 against style 64x48: the heights are ragged against
# conv1_1's 16-row tiles, Ns != Nc, and 3200 rows are 13 K-slices of 256 with a ragged last one (3072 rows: 12 full slices).
CASES = {
    'l1_a06_tf': ('c40x80', 's64x48', L1, 0.6, 'tf'),
    'l1_a10_tf': ('c40x80', 's64x48', L1, 1.0, 'tf'),
    'l1_a06_np': ('c40x80', 's64x48', L1, 0.6, 'np'),
    'l1_a10_np': ('c40x80', 's64x48', L1, 1.0, 'np'),
    'l21_a06_tf': ('c40x80', 's64x48', L21, 0.6, 'tf'),      # level 1 encodes a decoded image, with the clamp on
    'l21_a10_np': ('c40x80', 's64x48', L21, 1.0, 'np'),
    'five_64': ('c64x64', 's64x64', L5, 0.6, 'tf'),
    'batch3_styles': ('c3x40x80', 's3x64x48', L21, 0.6, 'tf'),
    'batch3_shared': ('c3x40x80', 's64x48', L21, 0.6, 'tf'),
    'batch3_l1_np': ('c3x40x80', 's3x64x48', L1, 1.0, 'np'),
    'tiny_16': ('c16x16', 's16x16', L1, 0.6, 'tf'),          # smaller than a tile on every side, one ragged K-slice
    'tiny_16_l21': ('c16x16', 's16x16', L21, 1.0, 'tf'),
    'rows_48x16': ('c48x16', 's16x16', L1, 0.6, 'np'),       # a 32-row stage spans two image rows
    'ragged_25x16': ('c25x16', 's16x16', L1, 1.0, 'tf'),     # 400 rows: the last K-slice ends 16 rows into a 32-row stage
    'content_w72': ('c40x72', 's64x48', L1, 0.6, 'tf'),      # a width that is no multiple of 16: the stored-feature path
    'style_w72': ('c40x80', 's64x72', L21, 0.6, 'tf'),
}


def make_inputs():
    rng = np.random.default_rng(20241)
    img = lambda *shape: rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    return {'c40x80': img(1, 40, 80), 's64x48': img(64, 48), 'c64x64': img(1, 64, 64), 's64x64': img(64, 64),
            'c3x40x80': img(3, 40, 80), 's3x64x48': img(3, 64, 48), 'c16x16': img(1, 16, 16), 's16x16': img(16, 16),
            'c48x16': img(1, 48, 16), 'c25x16': img(1, 25, 16), 'c40x72': img(1, 40, 72), 's64x72': img(64, 72)}


def run_cases(ctx, inputs):
    return {name: ctx.stylize_batch(inputs[ck], inputs[sk], levels, alpha=alpha, wct_mode=mode)
            for name, (ck, sk, levels, alpha, mode) in CASES.items()}


def _context():
    from wct_tf_amd.context import Context
    from wct_tf_amd.weights import synthetic_weights
    c = Context(0)
    c.set_weights(synthetic_weights(seed=42))
    return c


if __name__ == '__main__':          # the reference child: python <this file> <inputs.npz> <outputs.npz>
    assert os.environ.get('WCT_L1_FROM_IMAGE') == '0'
    d = np.load(sys.argv[1])
    np.savez(sys.argv[2], **run_cases(_context(), {k: d[k] for k in d.files}))
    sys.exit(0)


@pytest.fixture(scope='module')
def ctx():
    c = _context()
    yield c
    c.close()


@pytest.fixture(scope='module')
def inputs():
    return make_inputs()


@pytest.fixture(scope='module')
def reference(inputs, tmp_path_factory):
    """the frames of every case on the stored-feature path, computed once"""
    d = tmp_path_factory.mktemp('level1_image')
    np.savez(d / 'in.npz', **inputs)
    subprocess.run([sys.executable, os.path.abspath(__file__), str(d / 'in.npz'), str(d / 'out.npz')], check=True,
                   env=dict(os.environ, WCT_L1_FROM_IMAGE='0'), timeout=600)
    z = np.load(d / 'out.npz')
    return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def frames(ctx, inputs):
    assert os.environ.get('WCT_L1_FROM_IMAGE', '1') != '0'
    return run_cases(ctx, inputs)


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(CASES))
def test_frames_equal_the_stored_feature_path(name, frames, reference):
    got, want = frames[name], reference[name]
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), (name, int(np.abs(got.astype(int) - want.astype(int)).max()), float((got != want).mean()))
    assert got.std() > 1                                             # (frames, not a constant)
    if got.shape[0] == 3:
        assert len({f.tobytes() for f in got}) == 3


def _l1_profile(ctx, content, style):
    ctx.prof_enable(True)
    ctx.prof_reset()
    ctx.stylize_batch(content, style, L1, alpha=0.6)
    p = ctx.prof_read()
    ctx.prof_enable(False)
    return p


@pytest.mark.gpu
def test_level_1_moves_no_64_channel_fp32_map(ctx, inputs):
    """Engagement, by the per-class profile of a [relu1_1] call: both conv1_1 passes are charged the image and the unit sums alone
    (12 + 64 * 4 / 16 bytes a pixel), the covariance the images and the unit sums of both sides, the apply the content images and
    its fp16 output -- no 256-byte rows anywhere."""
    nc, ns = 40 * 80, 64 * 48
    p = _l1_profile(ctx, inputs['c40x80'], inputs['s64x48'])
    assert p['conv_first']['launches'] == 2
    assert p['conv_first']['bytes'] == (nc + ns) * (12 + 16)
    assert p['wct_cov']['bytes'] == (nc + ns) * (12 + 16)
    assert p['wct_apply']['bytes'] == nc * (12 + 128)
    assert p['conv12']['launches'] == 0                                         # (relu1_1 alone: no conv1_2)


@pytest.mark.gpu
def test_a_width_off_the_16_grid_keeps_the_stored_maps(ctx, inputs):
    nc, ns = 40 * 72, 64 * 48
    p = _l1_profile(ctx, inputs['c40x72'], inputs['s64x48'])
    assert p['conv_first']['launches'] == 2
    assert p['conv_first']['bytes'] == (nc + ns) * (12 + 256)
    assert p['wct_cov']['bytes'] == (nc + ns) * 2 * 256
    assert p['wct_apply']['bytes'] == nc * (256 + 128)
