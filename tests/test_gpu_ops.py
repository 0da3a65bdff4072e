"""GPU parity tests, op level: every call goes through the C ABI (libwct_hip.so) and is
checked against the CPU oracle on the same seeded inputs.

Tolerances (written here, from BASELINE.json's north star): WCT vs the reference NumPy
path <= 1e-3 relative in fp32.  Convolutions run fp16 operands / fp32 accumulate: against
an oracle fed the same fp16-rounded operands they must agree to accumulation-order noise
(2e-4); against the pure-fp32 oracle the fp16 operand rounding shows (<= 3e-3)."""
import os

import numpy as np
import pytest

import oracle
from conftest import GOLDEN, rel_err, max_rel, check_against_size_digest
from eig_cases import graded_spd as _graded_spd
from wct_tf_amd import _lib
from wct_tf_amd.weights import synthetic_features, synthetic_weights, synthetic_image

pytestmark = pytest.mark.gpu

WCT_TOL = 1e-3


@pytest.fixture(scope='module')
def ctx():
    from wct_tf_amd.context import Context
    c = Context(0)
    yield c
    c.close()


@pytest.mark.parametrize('c', [32, 64, 128, 256, 512])
def test_eigh_matches_lapack(ctx, c):
    rng = np.random.default_rng(c)
    mats = np.stack([_graded_spd(rng, c, 3.0), _graded_spd(rng, c, 1.0, rank=c // 3)])
    evals, evecs, sweeps = ctx.eigh(mats, return_sweeps=True)
    print('C=%d sweeps=%s' % (c, sweeps))
    assert max(sweeps) <= 14                  # two inside the budget of 16 (csrc/eigh.hip JACOBI_MAX_SWEEPS)
    for a, lam, v in zip(mats, evals, evecs):
        a64 = a.astype(np.float64)
        ref = np.linalg.eigvalsh(a64)
        norm = np.abs(ref).max()
        v64 = v.astype(np.float64)
        ev_err = np.abs(np.sort(lam) - ref).max() / norm
        orth = np.abs(v64.T @ v64 - np.eye(c)).max()
        resid = np.linalg.norm(a64 @ v64 - v64 * lam.astype(np.float64)) / np.linalg.norm(a64)
        print('  eig err/norm %.2e  orth %.2e  resid %.2e' % (ev_err, orth, resid))
        # fp32 two-sided Jacobi: a few hundred block updates leave ~1e-4 relative on the diagonal
        assert ev_err <= 2e-4 and orth < 2e-4 and resid < 2e-4


def test_eigh_small_eigenvalues_keep_relative_accuracy(ctx):
    # graded matrix: eigenvalues over 7 decades; the 1e-5 cut-off of ops.py:68-69 needs the
    # small ones resolved to far better than eps*||A||
    rng = np.random.default_rng(5)
    c = 128
    q, _ = np.linalg.qr(rng.standard_normal((c, c)))
    d = 10.0 ** np.linspace(2, -5, c)
    scale = 10.0 ** rng.uniform(-0.5, 0.5, c)
    a = ((q * d) @ q.T)
    a = (a * scale[:, None] * scale[None, :]).astype(np.float32)
    evals, _ = ctx.eigh(a)
    ref = np.linalg.eigvalsh(a.astype(np.float64))
    got = np.sort(evals[0])
    big = ref > 1e-5
    err = np.abs(got[big] - ref[big])
    print('  small-eig rel err', (err / ref[big])[:6], 'large', (err / ref[big])[-3:])
    assert np.all(err <= 2e-4 * ref[big] + 1e-8 * ref.max()), (err / (2e-4 * ref[big] + 1e-8 * ref.max())).max()


def test_eigensolver_failures_are_loud(ctx):
    """a solve that runs out of sweeps used to return whatever A/V held, with rc 0.  Now: the call still
    writes its outputs, returns WCT_STATUS_NOCONV (WCTNotConverged here), and sweeps_out carries -sweeps for the
    matrices still rotating (<= -1000 for non-finite input) -- through wct_eigh, wct_transform and, for the
    asynchronous batch entry point, through the next wct_sync.  The sweep budget is 16; WCT_JACOBI_MAX_SWEEPS (read
    at every solve) lowers it so the path can be exercised: no symmetric matrix needs 16 cyclic sweeps."""
    from wct_tf_amd._lib import WCTNotConverged
    rng = np.random.default_rng(9)
    a = _graded_spd(rng, 128, 3.0)
    os.environ['WCT_JACOBI_MAX_SWEEPS'] = '2'
    try:
        with pytest.raises(WCTNotConverged, match='still rotating'):
            ctx.eigh(np.stack([a, np.eye(128, dtype=np.float32)]))
        assert list(ctx.last_sweeps) == [-2, 1]            # the identity is done after its first (idle) sweep
        fc = synthetic_features(11, 64, 16, 16, 2.0)
        fs = synthetic_features(12, 64, 16, 16, 2.0)
        with pytest.raises(WCTNotConverged):
            ctx.transform(fc.reshape(-1, 64), fs.reshape(-1, 64), 0.8, _lib.WCT_TF)
        assert list(ctx.last_sweeps) == [-2, -2]
    finally:
        del os.environ['WCT_JACOBI_MAX_SWEEPS']
    evals, _, sweeps = ctx.eigh(a, return_sweeps=True)     # the status does not stick
    assert sweeps[0] > 2 and np.abs(np.sort(evals[0]) - np.linalg.eigvalsh(a.astype(np.float64))).max() < 2e-4 * np.abs(a).max() * 128
    # non-finite input: one NaN in a covariance (e.g. an fp16 overflow upstream) must not come back as "converged"
    bad = a.copy()
    bad[5, 9] = bad[9, 5] = np.nan
    with pytest.raises(WCTNotConverged, match='non-finite'):
        ctx.eigh(np.stack([a, bad]))
    assert ctx.last_sweeps[0] > 0 and ctx.last_sweeps[1] <= -1000
    fc_bad = fc.copy()
    fc_bad[0, 3, 3, 7] = np.inf
    with pytest.raises(WCTNotConverged):
        ctx.transform(fc_bad.reshape(-1, 64), fs.reshape(-1, 64), 0.8, _lib.WCT_NP)
    _check_wct(ctx, fc, fs, 0.8, 'np')                     # and the context is usable afterwards


def _check_wct(ctx, fc, fs, alpha, mode, tol=WCT_TOL):
    c = fc.shape[-1]
    want = (oracle.wct_np if mode == 'np' else oracle.wct_tf)(fc, fs, alpha)
    got, sweeps = ctx.transform(fc.reshape(-1, c), fs.reshape(-1, c), alpha,
                                _lib.WCT_NP if mode == 'np' else _lib.WCT_TF, return_sweeps=True)
    got = got.reshape(want.shape)
    e2, em = rel_err(got, want), max_rel(got, want)
    print('C=%d Nc=%d Ns=%d alpha=%.2f mode=%s sweeps=%s rel=%.2e max=%.2e' % (
        c, fc.size // c, fs.size // c, alpha, mode, sweeps, e2, em))
    assert e2 < tol and em < 5 * tol
    return got


def test_wct_matches_reference_golden_outputs(ctx):
    z = np.load(os.path.join(GOLDEN, 'wct_np_reference.npz'))
    names = sorted({k.split('/')[0] for k in z.files})
    for n in names:
        alpha = float(z[n + '/alpha'])
        alpha = 0.6 if alpha < 0 else alpha           # reference default (ops.py:92)
        fc, fs, ref = z[n + '/content'], z[n + '/style'], z[n + '/out']
        c = fc.shape[-1]
        got = ctx.transform(fc.reshape(-1, c), fs.reshape(-1, c), alpha, _lib.WCT_NP).reshape(ref.shape)
        print(n, rel_err(got, ref), max_rel(got, ref))
        assert rel_err(got, ref) < WCT_TOL, n
        assert max_rel(got, ref) < 5 * WCT_TOL, n


@pytest.mark.parametrize('c,hc,wc,hs,ws', [
    (64, 32, 32, 24, 40),
    (128, 24, 24, 24, 24),
    (256, 20, 20, 16, 30),
    (512, 24, 24, 32, 32),
])
@pytest.mark.parametrize('mode', ['np', 'tf'])
def test_wct_synthetic_features(ctx, c, hc, wc, hs, ws, mode):
    fc = synthetic_features(10 + c, c, hc, wc, 2.0)
    fs = synthetic_features(20 + c, c, hs, ws, 2.0)
    _check_wct(ctx, fc, fs, 0.8, mode)


def test_wct_rank_deficient_and_alpha_edges(ctx):
    # N < C: the null space sits ~1e-8, far below the 1e-5 cut-off (SURVEY.md 7 hard part 2)
    fc = synthetic_features(31, 128, 6, 6, 1.0, rank=20)
    fs = synthetic_features(32, 128, 5, 7, 1.0, rank=20)
    _check_wct(ctx, fc, fs, 0.8, 'np')
    _check_wct(ctx, fc, fs, 0.8, 'tf')
    fc = synthetic_features(33, 64, 16, 16, 2.0)
    fs = synthetic_features(34, 64, 16, 16, 2.0)
    got0 = _check_wct(ctx, fc, fs, 0.0, 'tf')
    assert rel_err(got0, fc) < 1e-5                   # alpha=0 returns the content features
    _check_wct(ctx, fc, fs, 1.0, 'np')


@pytest.mark.parametrize('mode', ['np', 'tf'])
def test_wct_rank_deficient_features_whose_rounding_noise_is_above_the_cutoff(ctx, mode):
    """N < C pixels (84 / 78 of C = 256) at feature scales 10 .. 1e4: the C - N + 1 exact zeros of the covariance come out as rounding
    noise of ~1e-7 ||cov||, which from a feature scale of ~10 on is ABOVE the reference's absolute 1e-5 cut-off (ops.py:68-69 /
    112,125).  The exact outcome (the oracle in float64) drops them; the reference's float32 evaluation keeps them with gains of
    order one and lands 1e-4 .. 2e-3 from the exact outcome.  Round 6 found this path off by 0.14 .. 11.5 at scale 1e3 (the
    completion of the spectral functions summed over noise pairs with squared cosines of order one -- csrc/spectral.hip
    pair_resolved / spectral_cut, profiles/r06_noise_block.txt).  Bound: 1e-3, or four times what the reference's float32 loses."""
    c, hc, wc, hs, ws = 256, 12, 7, 13, 6
    fn = oracle.wct_np if mode == 'np' else oracle.wct_tf
    kw64 = {'dtype': np.float64} if mode == 'tf' else {}
    worst = 0.0
    for seed, log_scale, alpha in [(464496, 3.0, 0.23694110562368303), (1, 3.0, 1.0), (4, 3.0, 0.6), (2, 1.0, 1.0), (3, 2.0, 0.8), (5, 4.0, 1.0)]:
        rng = np.random.default_rng(seed)
        def feats(n, scale):
            g = rng.standard_normal((n, c)) @ (rng.standard_normal((c, c)) / np.sqrt(c))
            return np.float32(np.maximum(g, 0) * 10.0 ** rng.uniform(-0.7, 0.7, c) * scale)
        fc = feats(hc * wc, 10.0 ** log_scale)
        fs = feats(hs * ws, 10.0 ** log_scale * 10.0 ** rng.uniform(-1, 1))
        got = ctx.transform(fc, fs, alpha, _lib.WCT_NP if mode == 'np' else _lib.WCT_TF)
        sh = (fc.reshape(1, hc, wc, c), fs.reshape(1, hs, ws, c))
        o64 = np.asarray(fn(np.float64(sh[0]), np.float64(sh[1]), alpha, **kw64)).reshape(-1, c)
        o32 = np.asarray(fn(*sh, alpha)).reshape(-1, c)
        mine, ref = rel_err(got, o64), rel_err(o32, o64)
        print('rank-deficient, scale 1e%d, alpha %.2f, %s: this path %.2e from the exact outcome, the reference in float32 %.2e' % (log_scale, alpha, mode, mine, ref))
        assert mine < max(WCT_TOL, 4 * ref), (seed, log_scale, alpha, mode, mine, ref)
        worst = max(worst, mine)
    assert worst < 5e-3


def test_wct_config_sizes(ctx):
    # BASELINE configs 1 and 2: (C,N) = (64, 65536) and (256, 16384); plus relu5_1 at 512^2
    for c, h, w in [(64, 256, 256), (256, 128, 128), (512, 32, 32)]:
        fc = synthetic_features(40 + c, c, h, w, 2.0)
        fs = synthetic_features(50 + c, c, h, w, 2.0)
        _check_wct(ctx, fc, fs, 0.8 if c != 64 else 1.0, 'np')


def test_wct_matches_reference_at_config_sizes(ctx):
    """BASELINE configs 2-4: the five WCT shapes of a 512x512 frame, (C, N) = (512,1024) (512,4096) (256,16384)
    (128,65536) (64,262144).  wct_np semantics against the digest of the REFERENCE's own wct_np run at that size
    (tests/golden/wct_np_sizes.npz, ops.py:92-140); wct_tf semantics against the oracle (ops.py:24-90).
    Tolerance: 1e-3 relative (north star), on the sampled rows, on the +-1 sketch over all pixels and on the
    per-channel moments."""
    from oracle.make_golden import SIZE_CASES, size_case_inputs, in_probe
    z = np.load(os.path.join(GOLDEN, 'wct_np_sizes.npz'))
    for case in SIZE_CASES:
        name, c, h, w, alpha = case[:5]
        fc, fs = size_case_inputs(case)
        assert np.allclose(np.stack([in_probe(fc), in_probe(fs)]), z[name + '/in_probe'], rtol=1e-6), name
        got, sweeps = ctx.transform(fc.reshape(-1, c), fs.reshape(-1, c), alpha, _lib.WCT_NP, return_sweeps=True)
        errs = check_against_size_digest(z, case, got, WCT_TOL)
        want = oracle.wct_np(fc, fs, alpha)          # pinned to the same digest in tests/test_oracle.py
        e_full = rel_err(got.reshape(want.shape), want)
        print('%s sweeps=%s rows %.2e sketch %.2e sq %.2e | full output vs oracle %.2e' % ((name, sweeps) + errs + (e_full,)))
        assert e_full < WCT_TOL and max_rel(got.reshape(want.shape), want) < 5 * WCT_TOL
        _check_wct(ctx, fc, fs, alpha, 'tf')


def test_wct_matches_reference_on_defective_and_real_image_features(ctx):
    """Exactly dead channels, exactly duplicated channels, 80 %-sparse post-ReLU maps, and features of the reference's
    sample photo (relu3_1 and the rank-deficient relu4_1: 144 pixels, 512 channels): wct_np semantics against the
    reference's own outputs (tests/golden/wct_np_hard.npz), wct_tf semantics against the oracle."""
    z = np.load(os.path.join(GOLDEN, 'wct_np_hard.npz'))
    names = sorted({k.split('/')[0] for k in z.files})
    assert len(names) == 5
    for n in names:
        fc, fs, ref, alpha = z[n + '/content'], z[n + '/style'], z[n + '/out'], float(z[n + '/alpha'])
        c = fc.shape[-1]
        got, sweeps = ctx.transform(fc.reshape(-1, c), fs.reshape(-1, c), alpha, _lib.WCT_NP, return_sweeps=True)
        got = got.reshape(ref.shape)
        print('%s C=%d sweeps=%s rel %.2e max %.2e' % (n, c, sweeps, rel_err(got, ref), max_rel(got, ref)))
        assert np.all(np.isfinite(got)), n
        assert rel_err(got, ref) < WCT_TOL and max_rel(got, ref) < 5 * WCT_TOL, n
        _check_wct(ctx, fc, fs, alpha, 'tf')


def test_wct_hard_512_channel_spectra_match_the_reference(ctx):
    """512-channel covariances graded over 5 decades at N = 4096, and N = 256 < C (6-decade grading; relu5_1 shape of a
    256x256 input): wct_np semantics against the reference's own outputs (tests/golden/wct_np_hard512.npz), wct_tf
    semantics against the oracle; the sweeps must stay two inside the budget of 16."""
    from oracle.make_golden import HARD512_CASES, hard512_inputs, in_probe
    z = np.load(os.path.join(GOLDEN, 'wct_np_hard512.npz'))
    for case in HARD512_CASES:
        name, c, h, w, alpha = case[:5]
        fc, fs = hard512_inputs(case)
        assert np.allclose(np.stack([in_probe(fc), in_probe(fs)]), z[name + '/in_probe'], rtol=1e-6), name
        got, sweeps = ctx.transform(fc.reshape(-1, c), fs.reshape(-1, c), alpha, _lib.WCT_NP, return_sweeps=True)
        errs = check_against_size_digest(z, case[:7], got, WCT_TOL)
        print('%s sweeps=%s rows %.2e sketch %.2e sq %.2e' % ((name, sweeps) + errs))
        assert 0 < min(sweeps) and max(sweeps) <= 14
        _check_wct(ctx, fc, fs, alpha, 'tf')


def test_wct_512_channel_spectrum_through_the_cutoff_within_the_kept_count_band(ctx):
    """C = 512, N = 4096, eigenvalues running THROUGH the 1e-5 cut-off with ~125 of them within a decade
    of it (tests/golden/wct_np_cross512.npz, a run of the reference's own wct_np).  Which borderline modes are kept is
    decided by fp32 rounding in the reference's SVD (eps ||A|| ~ 1e-6 against a 3.7 % eigenvalue spacing at 1e-5), so the
    output is judged like the fuzz tests judge C <= 128: it must equal the oracle for SOME kept counts within +-3 of the
    reference's own, to the tolerance the reference's fp32-vs-fp64 indeterminacy on this input allows.  This is also the
    regime in which the second-order completion of the spectral functions is switched off (a diagonal within half a
    decade of the cut-off), i.e. the slower, first-order path of the solver."""
    from oracle.make_golden import CROSS512_CASE, cross512_inputs, in_probe
    z = np.load(os.path.join(GOLDEN, 'wct_np_cross512.npz'))
    name, c, h, w, alpha = CROSS512_CASE[:5]
    fc, fs = cross512_inputs()
    assert np.allclose(np.stack([in_probe(fc), in_probe(fs)]), z[name + '/in_probe'], rtol=1e-6)
    kc0, ks0 = (int(k) for k in z[name + '/kept_reference'])
    for mode, fn, flag in (('np', oracle.wct_np, _lib.WCT_NP), ('tf', oracle.wct_tf, _lib.WCT_TF)):
        got, sweeps = ctx.transform(fc.reshape(-1, c), fs.reshape(-1, c), alpha, flag, return_sweeps=True)
        assert np.all(np.isfinite(got)) and 0 < min(sweeps) and max(sweeps) <= 14
        got = got.reshape(fc.shape)
        o32 = fn(fc, fs, alpha)
        o64 = fn(np.float64(fc), np.float64(fs), alpha, **({'dtype': np.float64} if mode == 'tf' else {}))
        own = rel_err(o32, o64)
        # coordinate search over the band (the two sides are nearly independent): content count first, then style
        errs = {}
        for kc in range(kc0 - 3, kc0 + 4):
            errs[(kc, ks0)] = rel_err(got, fn(fc, fs, alpha, keep=(kc, ks0)))
        kc_b = min(errs, key=errs.get)[0]
        for ks in range(ks0 - 3, ks0 + 4):
            errs[(kc_b, ks)] = rel_err(got, fn(fc, fs, alpha, keep=(kc_b, ks)))
        best = min(errs, key=errs.get)
        tol = max(WCT_TOL, 4 * own)
        print('  mode %s sweeps %s: reference kept (%d, %d), best match kept %s rel %.2e; at the reference counts %.2e; '
              'reference fp32 vs fp64 on this input %.2e' % (mode, sweeps, kc0, ks0, best, errs[best], errs[(kc0, ks0)], own))
        assert errs[best] < tol, (mode, errs, own)
    if True:
        # wct_np semantics also against the digest of the reference's own output when the counts agree
        got = ctx.transform(fc.reshape(-1, c), fs.reshape(-1, c), alpha, _lib.WCT_NP)
        if rel_err(got.reshape(fc.shape), oracle.wct_np(fc, fs, alpha)) < WCT_TOL:
            check_against_size_digest(z, CROSS512_CASE, got, WCT_TOL)


def test_wct_tf_mode_matches_the_reference_pin(ctx):
    """wct_tf semantics (ops.py:24-90) against the reference's wct_np(eps=0) + (1 - alpha) mc (tests/test_oracle.py
    explains the pin): the 1e-8 on the covariance diagonal is worth 0.5e-8 / lambda_min, far inside the 1e-3."""
    z = np.load(os.path.join(GOLDEN, 'wct_tf_reference.npz'))
    names = sorted({k.split('/')[0] for k in z.files})
    assert len(names) == 3
    for n in names:
        fc, fs, ref, alpha = z[n + '/content'], z[n + '/style'], z[n + '/out'], float(z[n + '/alpha'])
        c = fc.shape[-1]
        got = ctx.transform(fc.reshape(-1, c), fs.reshape(-1, c), alpha, _lib.WCT_TF).reshape(ref.shape)
        print('%s rel %.2e max %.2e' % (n, rel_err(got, ref), max_rel(got, ref)))
        assert rel_err(got, ref) < WCT_TOL and max_rel(got, ref) < 5 * WCT_TOL, n


def _graded_features(rng, n, c, decades):
    """Channels with log-spaced scales over `decades` and mild mixing: a graded covariance D H D with a
    well-conditioned H, the structure real feature maps have (tiny-variance channels), for which fp32
    arithmetic -- the reference's as much as ours -- keeps the small eigenvalues to high RELATIVE accuracy."""
    mix = np.eye(c) + 0.3 * rng.standard_normal((c, c)) / np.sqrt(c)
    d = 10.0 ** (-np.arange(c) * decades / (c - 1) / 2)
    return np.maximum(rng.standard_normal((n, c)) @ mix + 0.3, 0) * d


def test_wct_cutoff_straddle(ctx):
    """SURVEY 7 hard part 2: the 1e-5 eigenvalue cut-off (ops.py:68-69 / 112,125).  The features are scaled so that
    the cut-off falls in the geometric middle of the gap between two neighbouring eigenvalues (each ~12 % away, far
    beyond fp32 noise on a graded matrix): one is kept with a gain of ~300, the next is dropped.  A solver that
    mis-places either changes the output by O(1/sqrt(kept)), a hundred times the tolerance."""
    rng = np.random.default_rng(77)
    c, h, w = 64, 48, 48
    for trial in range(3):
        feats = []
        for side in range(2):
            x = _graded_features(rng, h * w, c, 7.0)
            ev = np.sort(np.linalg.eigvalsh(np.cov(np.float32(x).astype(np.float64).T)))
            k = 8 + 5 * trial + side                     # put the cut-off between eigenvalues k-1 and k
            x = x * np.sqrt(1e-5 / np.sqrt(ev[k - 1] * ev[k]))
            x = np.float32(x)
            ev = np.sort(np.linalg.eigvalsh(np.cov(x.astype(np.float64).T)))
            lo, hi = ev[ev <= 1e-5].max(), ev[ev > 1e-5].min()
            assert lo < 0.93e-5 and hi > 1.07e-5, (lo, hi)
            print('  side %d: %d eigenvalues kept, neighbours of the cut-off %.3e / %.3e' % (side, (ev > 1e-5).sum(), lo, hi))
            feats.append(x.reshape(1, h, w, c))
        for mode in ('np', 'tf'):
            _check_wct(ctx, feats[0], feats[1], 0.8, mode)


def test_wct_cutoff_straddle_within_one_per_cent(ctx):
    """two eigenvalues 1 % above and 1 % below the 1e-5 cut-off.  The first-order completion of the spectral
    functions divides the solver's residual by that gap; it is clamped to its bound f_k / 2 (spectral_entry), so the
    output must stay finite and equal the oracle for the reference's kept count -- or, if fp32 noise moves one of the
    two across the line, for a neighbouring count."""
    rng = np.random.default_rng(99)
    c, h, w = 64, 40, 40
    feats = []
    for side in range(2):
        x = _graded_features(rng, h * w, c, 3.0)
        x[:, :-2] *= 0.3 / x[:, :-2].std()
        # two channels of variance 1.01 v and 0.99 v, made exactly uncorrelated with the others and with each other
        # (sample correlations of ~N^-1/2 would split the pair by several per cent)
        base = x[:, :-2] - x[:, :-2].mean(0)
        z = rng.standard_normal((h * w, 2))
        z -= z.mean(0)
        z -= base @ np.linalg.lstsq(base, z, rcond=None)[0]
        q, _ = np.linalg.qr(z)
        x[:, -2] = q[:, 0] * 1e-3 * np.sqrt(1.01 * (h * w - 1))
        x[:, -1] = q[:, 1] * 1e-3 * np.sqrt(0.99 * (h * w - 1))
        ev = np.sort(np.linalg.eigvalsh(np.cov(np.float32(x).astype(np.float64).T)))
        lo, hi = ev[0], ev[1]                                      # the pair: far below every other eigenvalue
        assert hi / lo < 1.06 and ev[2] > 20 * hi, (lo, hi, ev[2])
        x = np.float32(x * np.sqrt(1e-5 / np.sqrt(lo * hi)))
        ev = np.sort(np.linalg.eigvalsh(np.cov(x.astype(np.float64).T)))
        print('  side %d: pair at %.4e / %.4e, next %.2e, largest %.2e' % (side, ev[0], ev[1], ev[2], ev[-1]))
        assert ev[0] < 1e-5 < ev[1] and ev[1] / ev[0] < 1.06
        feats.append(x.reshape(1, h, w, c))
    for mode in ('np', 'tf'):
        fn = oracle.wct_np if mode == 'np' else oracle.wct_tf
        got, sweeps = ctx.transform(feats[0].reshape(-1, c), feats[1].reshape(-1, c), 0.8,
                                    _lib.WCT_NP if mode == 'np' else _lib.WCT_TF, return_sweeps=True)
        assert np.all(np.isfinite(got))
        errs = {(kc, ks): rel_err(got.reshape(1, h, w, c), fn(feats[0], feats[1], 0.8, keep=(kc, ks)))
                for kc in (c - 2, c - 1, c) for ks in (c - 2, c - 1, c)}
        best = min(errs, key=errs.get)
        print('  mode %s sweeps %s: best kept counts %s rel %.2e (reference count %d/%d: %.2e)' % (mode, sweeps, best, errs[best], c - 1, c - 1, errs[(c - 1, c - 1)]))
        assert errs[best] < WCT_TOL, (mode, errs)
        assert np.abs(got).max() < 10 * np.abs(fn(feats[0], feats[1], 0.8)).max()


def test_wct_ops_module_surface(ctx):
    from wct_tf_amd import ops
    fc = synthetic_features(61, 64, 12, 12, 2.0)
    fs = synthetic_features(62, 64, 10, 14, 2.0)
    out = ops.wct_np(fc, fs, ctx=ctx)                 # defaults alpha=0.6, eps=1e-5
    assert out.dtype == np.float32 and out.shape == fc.shape
    assert rel_err(out, oracle.wct_np(fc, fs)) < WCT_TOL
    out = ops.wct_tf(fc, fs, 0.5, ctx=ctx)
    assert rel_err(out, oracle.wct_tf(fc, fs, 0.5)) < WCT_TOL
    with pytest.raises(ValueError):
        ops.wct_np(np.zeros((2, 4, 4, 64), np.float32), fs, ctx=ctx)   # batch must be 1


def test_adain(ctx):
    from wct_tf_amd import ops
    for c, h, w in [(64, 40, 40), (512, 8, 8), (128, 33, 17)]:
        fc = synthetic_features(70 + c, c, h, w, 2.0)
        fs = synthetic_features(80 + c, c, h + 3, w + 1, 2.0)
        got = ops.adain(fc, fs, 0.7, ctx=ctx)
        want = oracle.adain(fc, fs, 0.7)
        print('adain', c, rel_err(got, want))
        assert rel_err(got, want) < 1e-5 and max_rel(got, want) < 1e-4


def _h(x):
    return np.asarray(x, np.float16).astype(np.float32)


@pytest.mark.parametrize('h,w,cin,cout,relu,up', [
    (32, 32, 64, 64, True, False),       # small tile config
    (64, 48, 64, 128, True, False),
    (37, 29, 128, 64, True, False),      # ragged edges
    (16, 16, 512, 512, True, False),     # deep K
    (20, 12, 256, 128, False, True),     # upsample folded into the loader, no ReLU
    (128, 128, 64, 64, True, False),     # several tile rows and columns (64 tiles of 16x16 are under the 256 of <16,64,4,1>: the 8-row tile)
    (96, 96, 128, 128, True, False),     # ... at 128 channels (36 tiles: the 8-row tile, two 64-channel blocks)
    (4, 4, 64, 64, True, True),
    (360, 376, 64, 64, True, False),     # 24 x 23 = 552 tiles of 16x16, ragged edge (24 x 12 = 288 tall 32x16 tiles are under the 512
                                         # the policy asks for: tests/test_gpu_pointwise.py runs the tall tile, on a batch)
    (184, 180, 64, 64, False, True),     # the 16x16 tile on 368 x 360 with the upsample folded in, no ReLU
])
def test_conv3x3(ctx, h, w, cin, cout, relu, up):
    rng = np.random.default_rng(h * 1000 + cin)
    x = np.maximum(rng.standard_normal((h, w, cin)), 0).astype(np.float32)
    wt = (rng.standard_normal((3, 3, cin, cout)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32) * 0.1
    got = ctx.conv3x3(x, wt, b, relu=relu, upsample=up)
    xin = oracle.upsample2x_nearest(x) if up else x
    want16 = oracle.conv3x3_reflect(_h(xin), _h(wt), b, relu)
    want32 = oracle.conv3x3_reflect(xin, wt, b, relu)
    e16, e32 = rel_err(got, want16), rel_err(got, want32)
    print('conv %dx%d %d->%d up=%d: vs fp16-operand oracle %.2e, vs fp32 oracle %.2e' % (h, w, cin, cout, up, e16, e32))
    assert got.shape == want32.shape
    assert e16 < 2e-4 and max_rel(got, want16) < 1e-3
    assert e32 < 3e-3


@pytest.mark.parametrize('h,w,cin,cout,relu,up,pool,batch', [
    (32, 32, 256, 256, True, False, False, 1),      # 16 x 16 tiles x 128 channels
    (64, 48, 256, 256, True, False, True, 2),       # fused 'same' max-pool (conv3_4), a batch
    (37, 29, 256, 256, True, False, False, 1),      # ragged edges, odd height: a pair-row with one row inside
    (37, 29, 256, 256, True, False, True, 1),       # ... pooled in ceil mode
    (16, 16, 512, 512, True, False, False, 1),      # deep K, small grid: the 8-row tiles
    (20, 12, 256, 256, False, True, False, 1),      # upsample folded into the loader, no ReLU
    (48, 80, 512, 256, True, False, False, 1),      # decoder's 512 -> 256
    (24, 40, 64, 64, True, False, False, 1),        # a shape the policy leaves on the direct kernel (algo 2 packs for the call)
    (40, 24, 128, 192, True, True, False, 2),       # 64-channel blocks
])
def test_conv3x3_reduced_flop_kernel(ctx, h, w, cin, cout, relu, up, pool, batch):
    """csrc/conv_wino.hip (Winograd F(2,3) along y, direct along x) against (a) the restatement with ITS roundings
    (fp16 filters U = G g, fp16 transformed rows, fp16 output): what is left is accumulation order and fp16 rounding flips;
    (b) the fp32 oracle: the per-layer gate of 1.5e-3 (measured on the CPU first, profiles/r06_winograd_error.txt);
    (c) the direct kernel through the same entry point, whose bits must be the round-5 path's.
    Every case here selects the <8,64,2,2> tile shape; test_gpu_pointwise.py::test_wino_conv holds <16,128,1,4,IL> and <8,128,1,4> too."""
    rng = np.random.default_rng(h * 1000 + cin + 7 * pool)
    x = np.maximum(rng.standard_normal((batch, h, w, cin)), 0).astype(np.float32)
    wt = (rng.standard_normal((3, 3, cin, cout)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32) * 0.1
    got = ctx.conv3x3_f16(x, wt, b, relu=relu, upsample=up, pool=pool, algo=2)
    direct = ctx.conv3x3_f16(x, wt, b, relu=relu, upsample=up, pool=pool, algo=1)
    for i in range(batch):
        xin = oracle.upsample2x_nearest(x[i]) if up else x[i]
        emu = oracle.conv3x3_reflect_wino_f16(xin, wt, b, relu)
        want32 = oracle.conv3x3_reflect(_h(xin), wt, b, relu)
        old = _h(ctx.conv3x3(x[i], wt, b, relu=relu, upsample=up))
        if pool:
            emu, want32, old = oracle.maxpool2x2_same(emu), oracle.maxpool2x2_same(want32), oracle.maxpool2x2_same(old)
        assert got[i].shape == want32.shape
        e_emu, e32, e_dir = rel_err(got[i], emu), rel_err(got[i], want32), rel_err(direct[i], want32)
        print('wino %dx%d %d->%d up=%d pool=%d: vs its own roundings %.2e, vs fp32 %.2e (direct kernel %.2e)' % (h, w, cin, cout, up, pool, e_emu, e32, e_dir))
        assert e_emu < 1e-4 and max_rel(got[i], emu) < 2e-3          # (one fp16 ulp of the largest value: a rounding flip)
        assert e32 < 1.5e-3
        assert np.array_equal(direct[i], old)                      # algo 1 == wct_conv3x3's kernel, rounded to fp16


def test_conv3x3_pipeline_choice_is_by_layer_shape(ctx):
    """algo 0 (what run_encoder / run_decoder launch) takes the reduced-FLOP kernel for the >= 256-channel layers and the direct
    one below, whatever the batch or the image size: a frame must not depend on the batch it is computed in."""
    rng = np.random.default_rng(11)
    for cin, cout, wide in [(256, 256, True), (512, 512, True), (512, 256, True), (128, 256, False), (256, 128, False), (64, 64, False)]:
        wt = (rng.standard_normal((3, 3, cin, cout)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
        b = np.zeros(cout, np.float32)
        for batch, h, w in [(1, 16, 16), (3, 32, 48)]:
            x = np.maximum(rng.standard_normal((batch, h, w, cin)), 0).astype(np.float32)
            y0 = ctx.conv3x3_f16(x, wt, b, algo=0)
            assert np.array_equal(y0, ctx.conv3x3_f16(x, wt, b, algo=2 if wide else 1)), (cin, cout, batch)
            assert np.array_equal(y0[0], ctx.conv3x3_f16(x[0], wt, b, algo=0))        # batch == single image
    # the three tile shapes of the reduced-FLOP kernel (picked from the grid size: 8 / 4 / 1 images of 64 x 64 at 256 -> 256 take
    # <16,128,1,4, interleaved> / <8,128,1,4> / <8,64,2,2>) accumulate in the same order: the same bits
    wt = (rng.standard_normal((3, 3, 256, 256)) * np.sqrt(2.0 / (9 * 256))).astype(np.float32)
    b = rng.standard_normal(256).astype(np.float32) * 0.1
    x = np.maximum(rng.standard_normal((8, 64, 64, 256)), 0).astype(np.float32)
    y8 = ctx.conv3x3_f16(x, wt, b, algo=0)
    assert np.array_equal(y8[:4], ctx.conv3x3_f16(x[:4], wt, b, algo=0))
    assert np.array_equal(y8[0], ctx.conv3x3_f16(x[0], wt, b, algo=0))
    y8p = ctx.conv3x3_f16(x, wt, b, pool=True, algo=0)
    assert np.array_equal(y8p[0], ctx.conv3x3_f16(x[0], wt, b, pool=True, algo=0))
    assert np.array_equal(y8p[0], oracle.maxpool2x2_same(y8[0]))


def test_maxpool(ctx):
    rng = np.random.default_rng(3)
    for h, w, c in [(8, 8, 64), (9, 7, 128), (1, 5, 8)]:
        x = _h(rng.standard_normal((h, w, c)))
        assert np.array_equal(ctx.maxpool(x), oracle.maxpool2x2_same(x))


def test_coral_matches_reference(ctx):
    from wct_tf_amd import ops
    z = np.load(os.path.join(GOLDEN, 'coral_reference.npz'))
    names = sorted({k.split('/')[0] for k in z.files})
    for n in names:
        src, tgt = z[n + '/source'], z[n + '/target']
        got64 = ops.coral_numpy(src / 255., tgt / 255., ctx=ctx)
        assert rel_err(got64, z[n + '/coral']) < 1e-9
        got8 = ops.preserve_colors_np(src, tgt, ctx=ctx)
        ref8 = z[n + '/preserve']
        diff = np.abs(got8.astype(int) - ref8.astype(int))
        assert diff.max() <= 1 and (diff > 0).mean() < 1e-3        # truncation at utils.py:89
    # config-5 sizes: 512^2 style onto a 1024^2 content
    s = synthetic_image(1, 512, 512)
    t = synthetic_image(2, 1024, 1024)
    got = ops.preserve_colors_np(s, t, ctx=ctx)
    want = oracle.preserve_colors_np(s, t)
    diff = np.abs(got.astype(int) - want.astype(int))
    assert diff.max() <= 1 and (diff > 0).mean() < 1e-3


@pytest.mark.parametrize('c,hc,wc,hs,ws,p,st', [
    (64, 12, 12, 10, 14, 3, 1),
    (512, 32, 32, 32, 32, 3, 1),       # relu5_1 of a 512x512 pair
    (128, 9, 11, 8, 8, 1, 1),
    (64, 11, 13, 9, 9, 3, 2),          # stride 2 on sizes that survive the round trip
    (512, 16, 16, 16, 16, 3, 1),       # N = 256 < C: rank-deficient covariances on both sides (relu5_1 of a 256x256 pair) -- the
    (512, 22, 22, 12, 20, 3, 1),       # case the refresh A <- V^T A0 V exists for (it was wired into launch_wct only)
])
def test_style_swap(ctx, c, hc, wc, hs, ws, p, st):
    from wct_tf_amd import ops
    fc = synthetic_features(90 + c, c, hc, wc, 1.5)
    fs = synthetic_features(95 + c, c, hs, ws, 1.5)
    want, margins = oracle.wct_style_swap(fc, fs, 0.6, p, st, return_margins=True)
    got = ops.wct_style_swap(fc, fs, 0.6, p, st, ctx=ctx)
    e = rel_err(got, want)
    # The patch match is an argmax over correlations of WHITENED features, which this path has to ~1e-4 (the transform's own
    # error on these features: 2.4e-4, tools/probe/r06_swap_margin.py): a match the oracle itself decides by less than 1e-3 of the
    # correlation may legitimately go to the runner-up.  Round 6: quantified with the oracle's margins instead of "< 1 % of the
    # pixels" -- every pixel that differs must lie in the p x p footprint of such a near-tie position, and nowhere else.
    diff = np.abs(got - want).max(-1).reshape(want.shape[-3:-1]) > 1e-3 * np.abs(want).max()      # [hc][wc] (the maps carry a batch axis of 1)
    near = np.zeros(diff.shape, bool)
    for y, x in zip(*np.nonzero(margins < 1e-3)):
        near[y * st:y * st + p, x * st:x * st + p] = True
    print('style_swap C=%d %dx%d p=%d st=%d: rel %.2e, pixels differing %d (positions the oracle decides by < 1e-3: %d of %d; smallest margin %.1e)'
          % (c, hc, wc, p, st, e, int(diff.sum()), int((margins < 1e-3).sum()), margins.size, margins.min()))
    assert got.shape == want.shape
    assert e < 1e-3 or not np.any(diff & ~near), int((diff & ~near).sum())
    assert diff.mean() < 0.05
    with pytest.raises(Exception):
        ops.wct_style_swap(synthetic_features(1, 64, 12, 12), fs[:, :9, :9, :64] if c == 64 else synthetic_features(2, 64, 9, 9), 0.6, 3, 2, ctx=ctx)   # 12 does not survive stride 2
