"""The eigensolver tests' case pool and judge (tests/eig_cases.py), held on the CPU: every pool matrix is what its name says,
float32 LAPACK's own solution passes the judge at the bound the GPU tests apply (the reference alone is inside it), and the judge
rejects a planted error of each kind."""
import numpy as np
import pytest

import eig_cases as ec

ORDERS = (96, 256, 320)          # 32-wide block pairs with an odd pair count, the V-pass order, 64-wide with an odd pair count
BOUND = 2e-4                     # tests/test_gpu_ops.py::test_eigh_matches_lapack, tests/test_gpu_eigh.py


@pytest.fixture(scope='module')
def pools():
    return {c: ec.pool(c, c) for c in ORDERS}


@pytest.fixture(scope='module')
def lapack32(pools):
    """float32 LAPACK's (evals, evecs) of every pool matrix"""
    return {(c, n): np.linalg.eigh(a) for c, p in pools.items() for n, a in p.items()}


@pytest.mark.parametrize('c', ORDERS)
def test_pool_matrices_are_float32_finite_and_bit_symmetric(pools, c):
    p = pools[c]
    assert tuple(p) == ec.NAMES
    for n, a in p.items():
        assert a.dtype == np.float32 and a.shape == (c, c), n
        assert np.isfinite(a).all(), n
        assert np.array_equal(a, a.T), n


@pytest.mark.parametrize('c', ORDERS)
def test_graded_cases_are_the_matrices_test_gpu_ops_solves(pools, c):
    # the helper moved out of tests/test_gpu_ops.py: the same generator state gives that test's two matrices, in its order
    rng = np.random.default_rng(c)
    k = c
    g = rng.standard_normal((4 * c, k)) @ rng.standard_normal((k, c)) / np.sqrt(k)
    g = g * 10.0 ** rng.uniform(-1.5, 1.5, c)
    first = (g.T @ g / (4 * c - 1)).astype(np.float32)
    k = c // 3
    g = rng.standard_normal((4 * c, k)) @ rng.standard_normal((k, c)) / np.sqrt(k)
    g = g * 10.0 ** rng.uniform(-0.5, 0.5, c)
    second = (g.T @ g / (4 * c - 1)).astype(np.float32)
    assert np.array_equal(pools[c]['graded3'], first)
    assert np.array_equal(pools[c]['rank_third'], second)


@pytest.mark.parametrize('c', ORDERS)
def test_pool_spectra_are_what_the_names_say(pools, c):
    p = pools[c]
    ev = {n: np.linalg.eigvalsh(a.astype(np.float64)) for n, a in p.items()}       # ascending
    eps = 2.0 ** -24

    # graded3: column scales over 3 decades, so the spectrum runs over at least 6 (the squares), evenly -- no gap of a decade
    # among the eigenvalues above 1e-6 ||A|| -- and on down to the rounding of the float32 cast
    lam = ev['graded3']
    span = np.log10(lam[-1] / np.abs(lam).min())
    top = lam[lam > 1e-6 * lam[-1]]
    print('C=%d graded3: %.1f decades, %d of %d above 1e-6 ||A||, largest step x%.1f' % (c, span, top.size, c, (top[1:] / top[:-1]).max()))
    assert span > 6.0 and top.size > c // 2 and (top[1:] / top[:-1]).max() < 10.0

    lam = ev['rank_third']                               # c // 3 eigenvalues carry the matrix, the rest is the cast's rounding
    big = lam > 1e-4 * lam[-1]
    print('C=%d rank_third: %d above 1e-4 ||A||, the rest within %.1e ||A||' % (c, big.sum(), np.abs(lam[~big]).max() / lam[-1]))
    assert big.sum() == c // 3
    assert np.abs(lam[~big]).max() < c * eps * lam[-1]
    assert np.log10(lam[-1] / lam[big][0]) < 3.0

    assert np.array_equal(p['identity'], np.eye(c, dtype=np.float32))
    assert not p['zero'].any()

    d = np.diag(p['diagonal'])
    assert np.array_equal(p['diagonal'], np.diag(d))
    assert np.array_equal(np.sort(d), (10.0 ** np.linspace(2, -5, c)).astype(np.float32)[::-1])
    assert not np.array_equal(d, np.sort(d)) and not np.array_equal(d, np.sort(d)[::-1])       # shuffled
    assert abs(np.log10(d.max() / d.min()) - 7.0) < 1e-3

    lam = ev['clustered']                                # the whole spectrum inside 1 + [0, 1e-4], up to the cast's rounding
    width = lam[-1] - lam[0]
    print('C=%d clustered: width %.3e around %.6f' % (c, width, lam.mean()))
    assert 0.8e-4 < width < 1.2e-4
    assert abs(lam[0] - 1.0) < 1e-5 and np.diff(lam).max() < 1e-5

    lam = ev['noisy_null']                               # c // 4 - 1 signal eigenvalues of the 1e3-scale features, then noise
    sig = lam > 1e3
    noise = np.abs(lam[~sig])
    print('C=%d noisy_null: %d signal eigenvalues %.2e .. %.2e; noise |.| median %.1e max %.1e, %d of %d above 1e-5, %d negative'
          % (c, sig.sum(), lam[sig][0], lam[-1], np.median(noise), noise.max(), (noise > 1e-5).sum(), noise.size, (lam < 0).sum()))
    assert sig.sum() == c // 4 - 1
    assert lam[sig][0] > 1e5
    assert noise.max() < 1e-5 * lam[-1]                  # noise of the float32 products, far below the signal ...
    assert np.median(noise) > 1e-5                       # ... and above the transform's absolute cut-off
    assert (noise > 1e-5).sum() > 0.9 * noise.size


def test_batch_cycles_the_pool_from_shift(pools):
    p = pools[96]
    names, mats = ec.batch(p, 17, 3)
    assert names == [ec.NAMES[(3 + i) % 7] for i in range(17)]
    assert mats.shape == (17, 96, 96) and mats.dtype == np.float32
    for n, a in zip(names, mats):
        assert np.array_equal(a, p[n])
    assert names[0] == 'diagonal' and names[4] == 'graded3'              # instant and slow matrices side by side
    assert {names.index(n) % 7 for n in ec.NAMES} == set(range(7))


@pytest.mark.parametrize('c', ORDERS)
def test_float32_lapack_is_inside_the_bound(pools, lapack32, c):
    for n, a in pools[c].items():
        lam, v = lapack32[c, n]
        assert lam.dtype == np.float32 and v.dtype == np.float32
        ev_err, orth, resid = ec.judge(a, lam, v)
        print('C=%d %-10s ev %.2e orth %.2e resid %.2e' % (c, n, ev_err, orth, resid))
        assert ev_err <= BOUND and orth < BOUND and resid < BOUND, n


def test_judge_measures_the_zero_matrix_absolutely():
    z = np.zeros((32, 32), np.float32)
    assert ec.judge(z, np.zeros(32, np.float32), np.eye(32, dtype=np.float32)) == (0.0, 0.0, 0.0)
    ev_err, orth, resid = ec.judge(z, np.full(32, 1e-3, np.float32), np.eye(32, dtype=np.float32))
    assert abs(ev_err - 1e-3) < 1e-9 and orth == 0.0 and abs(resid - 1e-3 * np.sqrt(32)) < 1e-8


def _bad(m):
    ev_err, orth, resid = m
    return not (ev_err <= BOUND and orth < BOUND and resid < BOUND)


# Which matrices can show which planted error: a wrong eigenvalue needs ||A|| > 0; exchanging two eigenvectors is an error only
# where their eigenvalues differ by more than the bound (not inside `identity` or `clustered`); V^T in the place of V is an error
# only where V is far from symmetric and the spectrum is spread (a dense matrix that is not `clustered`); a column that is too
# long shows in V^T V whatever the matrix.
NONZERO = tuple(n for n in ec.NAMES if n != 'zero')
SPREAD = ('graded3', 'rank_third', 'diagonal', 'noisy_null')
DENSE_SPREAD = ('graded3', 'rank_third', 'noisy_null')


@pytest.mark.parametrize('c', ORDERS)
def test_judge_rejects_a_scaled_eigenvalue(pools, lapack32, c):
    for n in NONZERO:
        lam, v = lapack32[c, n]
        lam = lam.copy()
        lam[-1] *= np.float32(1 + 1e-3)
        assert _bad(ec.judge(pools[c][n], lam, v)), n
        assert ec.judge(pools[c][n], lam, v)[0] > BOUND, n


@pytest.mark.parametrize('c', ORDERS)
def test_judge_rejects_swapped_eigenvectors(pools, lapack32, c):
    for n in SPREAD:
        lam, v = lapack32[c, n]
        v = v.copy()
        v[:, [0, c - 1]] = v[:, [c - 1, 0]]
        m = ec.judge(pools[c][n], lam, v)
        assert _bad(m) and m[2] >= BOUND and m[0] <= BOUND and m[1] < BOUND, (n, m)     # the residual alone sees it


@pytest.mark.parametrize('c', ORDERS)
def test_judge_rejects_a_scaled_eigenvector(pools, lapack32, c):
    for n in ec.NAMES:
        lam, v = lapack32[c, n]
        v = v.copy()
        v[:, c // 2] *= np.float32(1 + 1e-3)
        m = ec.judge(pools[c][n], lam, v)
        assert _bad(m) and m[1] >= BOUND, (n, m)


@pytest.mark.parametrize('c', ORDERS)
def test_judge_rejects_a_transposed_basis(pools, lapack32, c):
    for n in DENSE_SPREAD:
        lam, v = lapack32[c, n]
        m = ec.judge(pools[c][n], lam, np.ascontiguousarray(v.T))
        assert _bad(m) and m[2] >= BOUND and m[1] < BOUND, (n, m)
