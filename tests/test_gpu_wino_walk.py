"""conv3x3_wino_walk_kernel<16,128,1,4> (csrc/conv_wino.hip): one block per CU that WALKS its tiles -- the last K-chunk of a tile
stages chunk 0 of the block's next tile, so only a block's first tile has a prologue.

All cases go through ctx.conv3x3_f16(..., algo=2), which forces the Winograd kernel.  launch_conv3x3_wino takes the walking shape
when Cout % 128 == 0 and ceil(W/16) * ceil(H/16) * B * (Cout/128) >= 256 (tests/pointwise.py::wino_config restates it), and a block
takes more than one tile when that count exceeds the CU count -- 256 on the MI355X.  The cases have 300, 300 and 378 tiles (sizes are
OUTPUT sizes), so some blocks take two tiles and others one; both edges are ragged (72 = 4.5, 88 = 5.5, 90 = 5.6, 106 = 6.6 tiles),
and a block's second tile (its first + 256) lies in another image and, in case C (three channel tiles, 256 % 3 = 1), in another
channel tile than its first one: the walk crosses images and channel tiles.

  A  5 x 72 x 88            64 -> 256   2 chunks per tile: the next tile is staged while the tile's second chunk runs
  B  5 x 72 x 88 (36 x 44)  128 -> 256  the folded x2 upsample
  C  3 x 90 x 106           64 -> 384   ReLU + the fused ceil-mode pool, odd pooled size 45 x 53

What is checked needs no stored expectation: every tile shape of the Winograd kernels accumulates an output in the same order
(K-chunk, frequency f, kx, k-step; the bias first, in M1), so the batched call on the walking shape must equal, bit for bit, the B
calls on the single images -- which have fewer than 256 tiles and run on the one-tile 8-row shapes."""
import numpy as np
import pytest

import oracle
import pointwise as pw
from conftest import rel_err, max_rel

pytestmark = pytest.mark.gpu

#        B   H   W   up     pool   Cin  Cout relu  tiles
CASES = {
    'A': (5, 72, 88, False, False, 64, 256, True, 300),
    'B': (5, 72, 88, True, False, 128, 256, True, 300),
    'C': (3, 90, 106, False, True, 64, 384, True, 378),
}


@pytest.fixture(scope='module')
def ctx():
    from wct_tf_amd.context import Context
    c = Context(0)
    yield c
    c.close()


def operands(case):
    b, h, w, up, pool, cin, cout, relu, tiles = CASES[case]
    rng = np.random.default_rng(20260 + ord(case))
    hin, win = (h // 2, w // 2) if up else (h, w)
    x = np.maximum(rng.standard_normal((b, hin, win, cin)), 0).astype(np.float32)
    wt = (rng.standard_normal((3, 3, cin, cout)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
    bias = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    return x, wt, bias


@pytest.fixture(scope='module')
def batched(ctx):
    """The batched output of every case, computed once and shared (never modified)."""
    out = {}
    for case, (b, h, w, up, pool, cin, cout, relu, tiles) in CASES.items():
        x, wt, bias = operands(case)
        out[case] = ctx.conv3x3_f16(x, wt, bias, relu=relu, upsample=up, pool=pool, algo=2)
    return out


@pytest.mark.parametrize('case', sorted(CASES))
def test_case_runs_on_the_walking_shape_and_its_single_images_do_not(case):
    b, h, w, up, pool, cin, cout, relu, tiles = CASES[case]
    assert -(-w // 16) * -(-h // 16) * b * (cout // 128) == tiles and tiles > 256
    assert pw.wino_config(cout, b, h, w) == 'IL16' and pw.wino_config(cout, 1, h, w) != 'IL16'


@pytest.mark.parametrize('case', sorted(CASES))
def test_batch_equals_single_images_bit_for_bit(ctx, batched, case):
    b, h, w, up, pool, cin, cout, relu, tiles = CASES[case]
    x, wt, bias = operands(case)
    got = batched[case]
    assert got.shape == (b, (h + 1) // 2 if pool else h, (w + 1) // 2 if pool else w, cout)
    for i in range(b):
        one = ctx.conv3x3_f16(x[i], wt, bias, relu=relu, upsample=up, pool=pool, algo=2)
        same = np.array_equal(got[i], one)
        if not same:
            bad = np.argwhere(got[i] != one)
            print('wino walk %s image %d: %d elements differ, first at %s' % (case, i, len(bad), bad[0]))
        assert same, (case, i)


def test_one_image_against_the_emulation_of_the_kernels_roundings(batched):
    """Image 3 of case A (tiles 180 .. 239 of the walk: first tiles of some blocks, none a block's second) and image 4 (tiles 240 ..
    299: 256 .. 299 are second tiles) against oracle.conv3x3_reflect_wino_f16.  The bound is the one of
    tests/test_gpu_fuzz.py::test_conv3x3_reduced_flop_kernel_random_shapes for this kernel against this emulation:
    rel_err < 1e-4 + 2e-3 / sqrt(elements), max_rel < 2e-3."""
    x, wt, bias = operands('A')
    for i in (3, 4):
        emu = oracle.conv3x3_reflect_wino_f16(x[i], wt, bias, True)
        got = batched['A'][i]
        assert got.shape == emu.shape
        r, m = rel_err(got, emu), max_rel(got, emu)
        print('wino walk A image %d vs emulation: rel_err %.3g max_rel %.3g' % (i, r, m))
        assert r < 1e-4 + 2e-3 / np.sqrt(emu.size) and m < 2e-3, (i, r, m)


def test_second_call_returns_the_same_bits(ctx, batched):
    """A patch or a weight fragment left behind by a block's last tile must not reach the next launch."""
    b, h, w, up, pool, cin, cout, relu, tiles = CASES['A']
    x, wt, bias = operands('A')
    again = ctx.conv3x3_f16(x, wt, bias, relu=relu, upsample=up, pool=pool, algo=2)
    assert np.array_equal(again, batched['A'])
