"""The transform's statistics, covariance, blend and apply kernels held row by row and channel by channel (tests/transform_rows.py
has the case lists, the float64 restatement and the judges; tests/test_transform_rows_cpu.py shows that the judges reject a row
dropped from a sum, a wrong output row, a zeroed channel block and an un-mirrored covariance tile by ten bounds and more, and
that the float32 oracle sits inside a tenth of them).

  colsum_kernel / colsum_finish_kernel    both passes through ctx.adain (units of 16 rows, then rows_per_slab), the first through
                                          every ctx.transform as well
  cov_f16x2_kernel<64|128> / cov_finish   through ctx.transform at alpha = 1 with one spiked row or channel per case
  gemm_f32_kernel's blend, apply_f16x2    through ctx.transform at alpha = 0 (M = I, bias = mc: the output is the content)

Every case prints a line `transform_rows <list> <case>: gpu ...`; profiles/transform_rows_margins.txt keeps those of one run beside
the float32 oracle's.  The bounds are the project's own (1e-3 for the transform, 1e-5 for AdaIN), per row and per channel; five
cases are left out by name (tr.LEFT_OUT, with the figures and the cause) and held to the whole-map bound instead."""
import pytest

import transform_rows as tr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from wct_tf_amd.context import Context
    c = Context(0)
    yield c
    c.close()


def _mode(name):
    from wct_tf_amd import _lib
    return _lib.WCT_NP if name == 'np' else _lib.WCT_TF


def _held_wct(ctx, name, ident, fc, fs, mode):
    want, _ = tr.wct64(fc, fs, 1.0, mode)
    got, sweeps = ctx.transform(fc, fs, 1.0, _mode(mode), return_sweeps=True)
    r, rn, ce, cn, co, on = tr.judge(got, want)
    print('transform_rows %s %s: gpu row %.2e at %d ch %.2e at %d own %.2e at %d sweeps %s' % (name, ident, r, rn, ce, cn, co, on, sweeps))
    assert max(r, ce, co) < tr.WCT_TOL, (ident, r, rn, ce, cn, co, on)


def _held_adain(ctx, name, case):
    fc, fs = tr.adain_inputs(case)
    want = tr.adain64(fc, fs, tr.ADAIN_ALPHA)
    got = ctx.adain(fc, fs, tr.ADAIN_ALPHA)
    r, rn, ce, cn, co, on = tr.judge(got, want)
    print('transform_rows %s %s: gpu row %.2e at %d ch %.2e at %d own %.2e at %d' % (name, tr.adain_id(case), r, rn, ce, cn, co, on))
    assert max(r, ce, co) < tr.ADAIN_TOL, (case, r, rn, ce, cn, co, on)


@pytest.mark.parametrize('case', tr.APPLY_CASES, ids=tr.apply_id)
def test_apply_alone_returns_the_content(ctx, case):
    """alpha = 0 in `tf` mode: pixel blocks of 128 with 2, 3, 127 rows in the only block, exactly one block, one and two rows in
    the second and a third block of one row; channel blocks of 64 (C < 128) and 128 with ragged last ones at 32, 96 and 160."""
    fc, fs = tr.apply_inputs(case)
    got = ctx.transform(fc, fs, 0.0, _mode('tf'))
    r, at = tr.apply_ratio(got, fc)
    print('transform_rows apply %s: gpu worst %.3f at %s' % (tr.apply_id(case), r, at))
    assert r <= 1, (case, r, at)


def _kept(name, cases, ident):
    return [c for c in cases if '%s %s' % (name, ident(c)) not in tr.LEFT_OUT]


@pytest.mark.parametrize('case', _kept('rows', tr.row_cases(), tr.row_id), ids=tr.row_id)
def test_spike_rows_reach_the_means_and_the_covariance(ctx, case):
    fc, fs = tr.row_inputs(case)
    _held_wct(ctx, 'rows', tr.row_id(case), fc, fs, case[5])


@pytest.mark.parametrize('case', _kept('channels', tr.channel_cases(), tr.channel_id), ids=tr.channel_id)
def test_spike_channels_and_a_pair_across_the_tile_boundary(ctx, case):
    fc, fs = tr.channel_inputs(case)
    _held_wct(ctx, 'channels', tr.channel_id(case), fc, fs, case[6])


def test_cases_left_out_by_name_stay_inside_the_whole_map_bound(ctx):
    """tr.LEFT_OUT: at most one case in twenty, each a case of the lists, each still inside the whole-map 1e-3 of
    tests/test_gpu_ops.py and inside 1e-3 per row -- what they exceed is ch_err in one loud channel, from the eigensolver's early
    stop (the reasons stand beside the names)."""
    named = {'rows ' + tr.row_id(c): (tr.row_inputs(c), c[5]) for c in tr.row_cases()}
    named.update({'channels ' + tr.channel_id(c): (tr.channel_inputs(c), c[6]) for c in tr.channel_cases()})
    assert set(tr.LEFT_OUT) <= set(named)
    assert 20 * len(tr.LEFT_OUT) <= len(named) + len(tr.APPLY_CASES) + len(tr.adain_cases()) + len(tr.STALE_CASES)
    for ident in tr.LEFT_OUT:
        (fc, fs), mode = named[ident]
        want, _ = tr.wct64(fc, fs, 1.0, mode)
        got, sweeps = ctx.transform(fc, fs, 1.0, _mode(mode), return_sweeps=True)
        r, rn, ce, cn, co, on = tr.judge(got, want)
        fro = tr.frobenius(got, want)
        print('transform_rows left-out %s: gpu row %.2e at %d ch %.2e at %d own %.2e at %d whole map %.2e sweeps %s' % (
            ident.replace(' ', '-', 1), r, rn, ce, cn, co, on, fro, sweeps))
        assert fro < tr.WCT_TOL and r < tr.WCT_TOL, (ident, fro, r, rn)


@pytest.mark.parametrize('case', tr.adain_cases(), ids=tr.adain_id)
def test_adain_pins_both_statistics_passes(ctx, case):
    _held_adain(ctx, 'adain', case)


@pytest.mark.parametrize('item', tr.STALE_CASES, ids=tr.stale_id)
def test_stale_rows_behind_the_features_reach_no_sum(item):
    """A fresh context whose staging buffers first hold N + 96 rows of values 1e4 times larger: the case that follows reads its N
    rows and nothing behind them."""
    from wct_tf_amd.context import Context
    kind, case = item
    c = Context(0)
    try:
        sc, ss = tr.stale_inputs(kind, case)
        if case[0] % 32 == 0:                       # (the transform takes multiples of 32 channels, AdaIN of 4)
            c.transform(sc, ss, 1.0, _mode('tf'))
        c.adain(sc, ss, tr.ADAIN_ALPHA)
        if kind == 'wct':
            fc, fs = tr.row_inputs(case)
            _held_wct(c, 'stale', tr.row_id(case), fc, fs, case[5])
        else:
            _held_adain(c, 'stale', case)
    finally:
        c.close()
