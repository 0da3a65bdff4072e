"""The judges of tests/transform_rows.py, checked on the CPU: they can fail, and they do not fail on float32 rounding.

For every case of every list the GPU test uses (tests/test_gpu_transform_rows.py):
 * the float32 oracle (oracle.wct_np / oracle.wct_tf / oracle.adain) sits inside a TENTH of the bound, per row and per channel --
   a condition on the inputs: a case that misses it gets other inputs, not another bound;
 * every mutation of the float64 restatement, applied at the case's spike row or channel, leaves the bound by at least TEN times
   in its worst row or channel;
 * on the alpha = 1 lists both kept counts equal C and the smallest kept eigenvalue is at least 100 times the cut-off.
Each case prints `transform_rows <list> <case>: float32 oracle ...` (profiles/transform_rows_margins.txt keeps one run)."""
import numpy as np
import pytest

import oracle
import transform_rows as tr


def _map(x):
    """[N][C] as the 1 x H x W x C map the oracle takes (it has no use for H and W beyond their product; N must factor)."""
    n, c = x.shape
    h = next(k for k in range(int(n ** 0.5), 0, -1) if n % k == 0)
    assert h > 1, n
    return x.reshape(1, h, n // h, c)


def _oracle_wct(fc, fs, alpha, mode):
    return (oracle.wct_np if mode == 'np' else oracle.wct_tf)(_map(fc), _map(fs), alpha).reshape(fc.shape)


def _worst(got, want, tol):
    return tr.worst(got, want) / tol


def _check_wct_case(name, ident, fc, fs, mode, mutations):
    c = fc.shape[1]
    want, info = tr.wct64(fc, fs, 1.0, mode)
    assert info['kc'] == c and info['ks'] == c, (ident, info)
    assert min(info['wc_min'], info['ws_min']) >= 100 * tr.CUTOFF, (ident, info)
    r, rn, ce, cn, co, on = tr.judge(_oracle_wct(fc, fs, 1.0, mode), want)
    hit = {}
    for m in mutations:
        hit[m[0]] = _worst(tr.wct64(fc, fs, 1.0, mode, mutate=m)[0], want, tr.WCT_TOL)
    weakest = min(hit, key=hit.get)
    print('transform_rows %s %s: float32 oracle row %.2e at %d ch %.2e at %d own %.2e at %d, min eig %.1e / %.1e, weakest mutation %s %.1fx' % (
        name, ident, r, rn, ce, cn, co, on, info['wc_min'], info['ws_min'], weakest, hit[weakest]))
    assert max(r, ce, co) <= 0.1 * tr.WCT_TOL, (ident, r, rn, ce, cn, co, on)
    assert hit[weakest] >= 10, (ident, hit)


def _check_adain_case(name, case):
    fc, fs = tr.adain_inputs(case)
    side, row = case[3], case[4]
    assert (fc if side == 'c' else fs)[row].min() > 0, case            # no post-ReLU zero hides the row from a channel
    want = tr.adain64(fc, fs, tr.ADAIN_ALPHA)
    got = oracle.adain(fc[None, :, None, :], fs[None, :, None, :], tr.ADAIN_ALPHA).reshape(fc.shape)
    r, rn, ce, cn, co, on = tr.judge(got, want)
    hit = {m[0]: _worst(tr.adain64(fc, fs, tr.ADAIN_ALPHA, mutate=m), want, tr.ADAIN_TOL) for m in tr.adain_mutations(case)}
    weakest = min(hit, key=hit.get)
    print('transform_rows %s %s: float32 oracle row %.2e at %d ch %.2e at %d own %.2e at %d, weakest mutation %s %.1fx' % (
        name, tr.adain_id(case), r, rn, ce, cn, co, on, weakest, hit[weakest]))
    assert max(r, ce, co) <= 0.1 * tr.ADAIN_TOL, (case, r, rn, ce, cn, co, on)
    assert hit[weakest] >= 10, (case, hit)


# ---- the restatement is the oracle's transform --------------------------------------------------------------------------

@pytest.mark.parametrize('mode', ['np', 'tf'])
def test_restatement_matches_the_oracle_in_float64(mode):
    """oracle.wct_np follows its input's dtype and oracle.wct_tf takes dtype=float64: on float64 copies of the inputs they agree
    with wct64 to rounding (svd there, eigh here), at alpha = 1 and at a blend, so the two state the same transform."""
    fc, fs = tr.row_inputs(tr.row_cases()[3])
    for alpha in (1.0, 0.6):
        want, _ = tr.wct64(fc, fs, alpha, mode)
        if mode == 'np':
            ref = oracle.wct_np(np.float64(_map(fc)), np.float64(_map(fs)), alpha)
        else:
            ref = oracle.wct_tf(_map(fc), _map(fs), alpha, dtype=np.float64)
        ref = ref.reshape(fc.shape)                                     # (the oracle returns float32: 6e-8 of a value)
        assert np.abs(ref - want).max() <= 2.0 ** -22 * np.abs(want).max(), (mode, alpha)


def test_case_lists_cover_what_the_issue_names():
    rows = tr.row_cases()
    assert {c[:2] for c in rows} >= {(32, 289), (64, 289), (128, 529), (160, 513), (256, 529), (96, 545)}
    assert any(c[2] >= c[1] + 256 for c in rows) and any(c[1] >= c[2] + 256 for c in rows)
    for c, nc, ns in tr.ROW_SHAPES:
        for side, n in (('c', nc), ('s', ns)):
            assert {k[4] for k in rows if k[:4] == (c, nc, ns, side)} == {0, 7, 8, 15, 16, 31, 32, 255, 256, n - 2, n - 1}
    for side in 'cs':                       # every spike position meets both modes on either side
        for r in (0, 7, 8, 15, 16, 31, 32, 255, 256):
            assert {k[5] for k in rows if k[3] == side and k[4] == r} == {'np', 'tf'}, (side, r)
    ch = tr.channel_cases()
    for c in (96, 160, 256):
        for side in 'cs':
            assert {k[5] for k in ch if k[0] == c and k[3] == side and k[4] == 'spike'} == {p for p in (0, 31, 32, 63, 64, 127, 128, c - 1) if p < c}
    assert {(k[0], k[5]) for k in ch if k[4] == 'pair'} == {(96, 63), (160, 127), (256, 127)}
    assert tr.adain_nslab(16400, 33) == 256 and tr.adain_nslab(257, 4100) == 65
    # (32, 16400, 33): 1025 units, 5 per slab, 205 of 256 slabs used; 65 rows per slab, 253 of 256 used
    assert tr.adain_slab_rows(16400, 256) == ([16320, 16399], [16380, 16399])
    assert tr.adain_slab_rows(33, 256) == ([32, 32], [32, 32])
    assert tr.adain_slab_rows(1041, 17) == ([1024, 1040], [992, 1040])
    assert {c[:3] for c in tr.adain_cases()} == set(tr.ADAIN_SHAPES)
    assert set(tr.APPLY_CASES) == {(c, n) for c in (32, 64, 96, 128, 160, 256, 512) for n in (2, 3, 127, 128, 129, 257)}


# ---- Test 1 ---------------------------------------------------------------------------------------------------------------

def _tf_alpha0_float32(x):
    """The float32 arithmetic of oracle.wct_tf's last line at alpha = 0, 0 colored + 1 ((x - mc) + mc), for an [N][C] matrix: the
    oracle takes H x W maps, and 2, 3, 127 and 257 rows do not factor.  Held against the oracle where N factors."""
    xt = np.ascontiguousarray(np.asarray(x, np.float32).T)
    mc = xt.mean(axis=1, keepdims=True)
    return np.ascontiguousarray((np.float32(1) * ((xt - mc) + mc)).T)


@pytest.mark.parametrize('c', sorted({c for c, _ in tr.APPLY_CASES}))
def test_apply_cases(c):
    for case in [k for k in tr.APPLY_CASES if k[0] == c]:
        fc, fs = tr.apply_inputs(case)
        nc = case[1]
        got = _tf_alpha0_float32(fc)
        if nc in (128, 129):                                       # the oracle itself (36 style rows: 37 do not factor either)
            ref = _oracle_wct(fc, fs[:36], 0.0, 'tf')
            assert tr.apply_ratio(got, ref)[0] <= 0.125, case      # the helper is the oracle to an ulp of a value
            got = ref
        r, at = tr.apply_ratio(got, fc)
        bad_row = np.array(fc)
        bad_row[nc - 1] = fc[nc - 2]
        bad_blk = np.array(fc)
        bad_blk[:, c - 4:] = 0
        hr, hb = tr.apply_ratio(bad_row, fc)[0], tr.apply_ratio(bad_blk, fc)[0]
        print('transform_rows apply %s: float32 oracle %.3f at %s, |mc| / max|x| >= %.2f, wrong row %.0fx, zeroed block %.0fx' % (
            tr.apply_id(case), r, at, (fc.mean(0) / fc.max()).min(), hr, hb))
        assert r <= 0.1, (case, r, at)
        assert hr >= 10 and hb >= 10, (case, hr, hb)


# ---- Tests 2, 3 and 5 -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', tr.ROW_SHAPES, ids=lambda s: 'C%d-%dx%d' % s)
def test_row_cases(shape):
    for case in [k for k in tr.row_cases() if k[:3] == shape]:
        fc, fs = tr.row_inputs(case)
        _check_wct_case('rows', tr.row_id(case), fc, fs, case[5], tr.row_mutations(case))


@pytest.mark.parametrize('shape', tr.CHANNEL_SHAPES, ids=lambda s: 'C%d-%dx%d' % s)
def test_channel_cases(shape):
    for case in [k for k in tr.channel_cases() if k[:3] == shape]:
        fc, fs = tr.channel_inputs(case)
        _check_wct_case('channels', tr.channel_id(case), fc, fs, case[6], tr.channel_mutations(case))


def test_stale_cases_are_cases_of_the_lists():
    """What runs second in a stale-rows test is judged as in its own list; the first call differs in size and scale."""
    for kind, case in tr.STALE_CASES:
        assert case in (tr.row_cases() if kind == 'wct' else tr.adain_cases()), case
        sc, ss = tr.stale_inputs(kind, case)
        assert sc.shape == (case[1] + tr.STALE_ROWS, case[0]) and ss.shape == (case[2] + tr.STALE_ROWS, case[0])
        fc, fs = (tr.row_inputs if kind == 'wct' else tr.adain_inputs)(case)
        assert np.abs(sc).mean() > 1e3 * np.abs(fc).mean() and np.abs(ss).mean() > 1e3 * np.abs(fs).mean()


# ---- Test 4 -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', tr.ADAIN_SHAPES, ids=lambda s: 'C%d-%dx%d' % s)
def test_adain_cases(shape):
    for case in [k for k in tr.adain_cases() if k[:3] == shape]:
        _check_adain_case('adain', case)
