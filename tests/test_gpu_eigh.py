"""wct_eigh across what its entry point accepts: orders off the pipeline's four, batch sizes on either side of the V-pass
threshold, failures inside a V-pass batch, the upper-triangle contract, refusals.

The cases come from tests/eig_cases.py (held on the CPU by tests/test_eig_cases_cpu.py); accuracy is judged against float64 LAPACK
at the bounds of tests/test_gpu_ops.py::test_eigh_matches_lapack, and everything the code promises bit for bit -- a matrix does
not depend on its batch, the V pass writes the bits of the fused update, the lower triangle is never read -- is compared with
np.array_equal.  Every test prints the sweeps and the three measures it saw (profiles/eigh_entry_coverage.txt is that output)."""
import ctypes
import os

import numpy as np
import pytest

import eig_cases as ec
from wct_tf_amd._lib import WCTHipError, WCTNotConverged, check, fptr

pytestmark = pytest.mark.gpu

BOUND = 2e-4                     # test_eigh_matches_lapack's, set at C <= 512


@pytest.fixture(scope='module')
def ctx():
    from wct_tf_amd.context import Context
    c = Context(0)
    yield c
    c.close()


_POOLS = {}


def _pool(c):
    if c not in _POOLS:
        _POOLS[c] = ec.pool(c, c)
    return _POOLS[c]


@pytest.fixture(scope='module')
def solo(ctx):
    """solo(c) -> {name: (evals [c], evecs [c][c], sweeps)}: every pool matrix of order c solved alone (nmat = 1), once"""
    cache = {}

    def get(c):
        if c not in cache:
            cache[c] = {}
            for n, a in _pool(c).items():
                lam, v, sw = ctx.eigh(a, return_sweeps=True)
                cache[c][n] = (lam[0], v[0], sw[0])
        return cache[c]
    return get


def _path(c, nmat):
    """the path csrc/eigh.hip takes (jacobi_dispatch, jacobi_run_fused, vstrip_launch), for the printed record only"""
    width = 64 if c % 64 == 0 and c >= 256 else 32
    vpass = width == 64 and c in (256, 512) and nmat >= 24
    return '%d-wide pairs x%d, %s' % (width, c // width, ('V pass, %s-major grid' % ('matrix' if nmat % 8 == 0 else 'strip'))
                                      if vpass else 'V in the fused update')


def _raw_eigh(ctx, a):
    """wct_eigh on [n][c][c] as given -> (rc, evals, evecs, sweeps): the outputs of a call that reports a failure"""
    n, c, _ = a.shape
    evals = np.empty((n, c), np.float32)
    evecs = np.empty((n, c, c), np.float32)
    sweeps = (ctypes.c_int * n)()
    rc = ctx.lib.wct_eigh(ctx.h, fptr(a), c, n, fptr(evals), fptr(evecs), sweeps)
    return rc, evals, evecs, list(sweeps)


def _assert_trivial_exact(name, a, lam, v):
    """A matrix that is already diagonal comes back EXACT: every column of V is a unit vector e_p (entries 0 and 1, one 1 per row
    and column), and column j carries the eigenvalue of its own direction, lam[j] == a[p_j][p_j] to the bit.  Returns p."""
    c = a.shape[0]
    assert np.isin(v, (0.0, 1.0)).all(), name
    assert (v.sum(axis=0) == 1).all() and (v.sum(axis=1) == 1).all(), name
    p = v.argmax(axis=0)
    assert np.array_equal(lam, np.diag(a)[p]), name
    assert np.array_equal(np.sort(lam), np.sort(np.diag(a))), name
    assert sorted(p) == list(range(c)), name
    return p


# ---- (a) orders off the pipeline's four ------------------------------------------------------------------------------------------
# 32-wide block pairs: 3, 5, 7, 9 of them (288: that path above 256 channels); 64-wide: 5, 6, 7 and, at the limit the residual
# tiles and row sums are sized for, 16
@pytest.mark.parametrize('c', [96, 160, 224, 288, 320, 384, 448, 1024])
def test_eigh_orders_off_the_pipeline(ctx, c):
    p = _pool(c)
    mats = np.stack([p['graded3'], p['rank_third']])
    evals, evecs, sweeps = ctx.eigh(mats, return_sweeps=True)
    measures = [ec.judge(a, lam, v) for a, lam, v in zip(mats, evals, evecs)]
    worst = np.max(measures, axis=0)                      # (a NaN stays a NaN)
    print('COVERAGE (a) C=%-4d nmat=2  graded3+rank_third  ev_err %.2e orth %.2e resid %.2e  sweeps %s  [%s]'
          % (c, worst[0], worst[1], worst[2], sweeps, _path(c, 2)))
    if c <= 512:
        assert max(sweeps) <= 14 and min(sweeps) > 0      # two inside the budget of 16, as test_eigh_matches_lapack
        bound = BOUND
    else:
        # rounding accumulates as a random walk over the rotations applied to an element, whose number per sweep grows with C:
        # the bound set at 512 scaled by sqrt(1024 / 512); converged inside the budget of 16
        assert min(sweeps) > 0
        bound = BOUND * np.sqrt(1024 / 512)
    for ev_err, orth, resid in measures:
        print('  eig err/norm %.2e  orth %.2e  resid %.2e' % (ev_err, orth, resid))
        assert ev_err <= bound and orth < bound and resid < bound


# ---- (b) a matrix does not depend on its batch -------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [128, 256, 384, 512])
def test_eigh_pool_solved_alone(solo, c):
    s = solo(c)
    measures = {n: ec.judge(a, s[n][0], s[n][1]) for n, a in _pool(c).items()}
    for n, m in measures.items():
        print('COVERAGE (b) C=%-4d nmat=1  %-10s  ev_err %.2e orth %.2e resid %.2e  sweeps %d  [%s]'
              % ((c, n) + m + (s[n][2], _path(c, 1))))
    for n, a in _pool(c).items():
        lam, v, sw = s[n]
        ev_err, orth, resid = measures[n]
        assert sw > 0, n
        assert ev_err <= BOUND and orth < BOUND and resid < BOUND, n
        if n in ec.TRIVIAL:
            p = _assert_trivial_exact(n, a, lam, v)
            rev = (np.arange(c) // 32) * 32 + 31 - np.arange(c) % 32
            print('  %-8s columns: %s' % (n, 'in place' if np.array_equal(p, np.arange(c)) else
                                          'each block of 32 reversed' if np.array_equal(p, rev) else 'another permutation'))


@pytest.mark.parametrize('c', [128, 256, 384, 512])
def test_eigh_trivial_matrices_come_back_in_place(solo, c):
    """identity, diagonal and zero come back exact and in place: evals == diag(A) position by position, V == I.

    On the 64-wide block pairs (C = 256, 384, 512 here) the intra step of a sweep (csrc/jacobi_pair64.h intra_wave) orders its
    pairs by odd-even transposition WITH EXCHANGE and leaves the 32 columns of every block in reverse order: until
    jacobi_unexchange_kernel (csrc/eigh.hip) these matrices, done after one sweep, came back with V the permutation that reverses
    each block of 32 columns and evals permuted alike (exact, but not in place)."""
    s = solo(c)
    for n in ec.TRIVIAL:
        a = _pool(c)[n]
        lam, v, sw = s[n]
        assert np.array_equal(lam, np.diag(a)), n                          # in place, unsorted
        assert np.array_equal(v, np.eye(c, dtype=np.float32)), n


@pytest.mark.parametrize('c', [128, 256, 384, 512])
def test_eigh_eigenpair_j_grows_out_of_coordinate_j(ctx, c):
    """The same order on a matrix that IS rotated, and for more than one sweep: d = 10 ** linspace(0, 6, c) on the diagonal and
    one coupling per coordinate, a[i][i + c/2] = 0.05 sqrt(d_i d_j).  The relative off-diagonal 0.05 is above the solver's
    stop tolerance (1e-2), so the first sweep cannot be the last; each 2 x 2 problem has d_j / d_i = 1e3, so by first-order
    perturbation theory eigenvector i leans 0.05 sqrt(d_i / d_j) = 1.6e-3 out of e_i and eigenvalue i moves by
    0.05^2 d_i (1 + 1e-3) = 2.5e-3 d_i at the most.  A column that belonged to another coordinate of its block would have
    |V[j][j]| near 0 and an eigenvalue off by its factor of 10 ** (6 / c) per place.  Solved beside `diagonal` (one sweep), so
    that the two matrices of the call end on sweep counts of their own."""
    d = 10.0 ** np.linspace(0, 6, c)
    a = np.diag(d)
    i = np.arange(c // 2)
    a[i, i + c // 2] = a[i + c // 2, i] = 0.05 * np.sqrt(d[i] * d[i + c // 2])
    a = a.astype(np.float32)
    assert np.array_equal(a, a.T)
    evals, evecs, sweeps = ctx.eigh(np.stack([a, _pool(c)['diagonal']]), return_sweeps=True)
    m = ec.judge(a, evals[0], evecs[0])
    lean = np.abs(np.diag(evecs[0])).min()
    move = (np.abs(evals[0] - np.diag(a)) / np.diag(a)).max()
    print('C=%d sweeps %s  ev_err %.2e orth %.2e resid %.2e  min |V[j][j]| %.6f  max |evals[j] - a[j][j]| / a[j][j] %.2e'
          % ((c, sweeps) + m + (lean, move)))
    assert sweeps[0] >= 2 and sweeps[1] == 1
    assert m[0] <= BOUND and m[1] < BOUND and m[2] < BOUND
    assert lean > 0.99 and move < 1e-2
    _assert_trivial_exact('diagonal', _pool(c)['diagonal'], evals[1], evecs[1])
    assert np.array_equal(evecs[1], np.eye(c, dtype=np.float32))


@pytest.mark.parametrize('c,nmat,shift', [
    (256, 23, 0), (256, 23, 3),        # the last batch size below the V pass
    (256, 24, 0), (256, 24, 3),        # V pass, matrix-major grid
    (256, 25, 0), (256, 25, 3),        # V pass, strip-major grid
    (256, 64, 0), (256, 64, 3),        # the ABI's limit
    (512, 24, 0),                      # V pass on 64-wide block pairs x8
    (512, 32, 2),
    (128, 64, 0),                      # 32-wide pairs, never the V pass: pure batch indexing
    (384, 24, 5),                      # 64-wide pairs without a V-pass instantiation
])
def test_eigh_batch_member_equals_solo_solve(ctx, solo, c, nmat, shift):
    s = solo(c)
    names, mats = ec.batch(_pool(c), nmat, shift)
    evals, evecs, sweeps = ctx.eigh(mats, return_sweeps=True)
    print('COVERAGE (b) C=%-4d nmat=%-2d shift=%d  sweeps %s  [%s]'
          % (c, nmat, shift, ' '.join('%s:%d' % (n, s[n][2]) for n in ec.NAMES), _path(c, nmat)))
    bad = [(i, n, what) for i, n in enumerate(names)
           for what, got, want in (('evals', evals[i], s[n][0]), ('evecs', evecs[i], s[n][1]), ('sweeps', sweeps[i], s[n][2]))
           if not np.array_equal(got, want)]
    for i, n, what in bad[:8]:
        if what == 'sweeps':
            print('  position %d (%s): sweeps %d, alone %d' % (i, n, sweeps[i], s[n][2]))
        else:
            got, want = (evals[i], s[n][0]) if what == 'evals' else (evecs[i], s[n][1])
            print('  position %d (%s): %s differ in %d of %d elements, max |diff| %.2e'
                  % (i, n, what, (got != want).sum(), got.size, np.abs(got.astype(np.float64) - want).max()))
    assert not bad, '%d of %d outputs differ from the solo solve' % (len(bad), 3 * nmat)


# ---- (c) failures inside a V-pass batch ------------------------------------------------------------------------------------------
def test_eigh_failures_inside_a_vpass_batch(ctx, solo):
    """tests/test_gpu_ops.py::test_eigensolver_failures_are_loud's contract at C = 256 with 25 matrices: the V pass on the side
    stream, strip-major grid, matrices that stop at different segments."""
    c, nmat = 256, 25
    s = solo(c)
    pool = _pool(c)
    names, mats = ec.batch(pool, nmat, 0)
    os.environ['WCT_JACOBI_MAX_SWEEPS'] = '2'
    try:
        rc, evals, evecs, sweeps = _raw_eigh(ctx, mats)
        print('COVERAGE (c) C=%-4d nmat=%d budget 2  sweeps %s  [%s]' % (c, nmat, sweeps, _path(c, nmat)))
        with pytest.raises(WCTNotConverged, match='still rotating'):
            check(rc)
        for i, n in enumerate(names):
            if n in ('graded3', 'rank_third'):
                assert sweeps[i] == -2, (i, n, sweeps[i])
            if n in ec.TRIVIAL:
                assert sweeps[i] > 0, (i, n, sweeps[i])
                _assert_trivial_exact(n, mats[i], evals[i], evecs[i])
                # done after one sweep whatever the budget: the bits of the solve with the full budget
                assert sweeps[i] == s[n][2] and np.array_equal(evals[i], s[n][0]) and np.array_equal(evecs[i], s[n][1]), (i, n)
    finally:
        del os.environ['WCT_JACOBI_MAX_SWEEPS']
    # non-finite input: one NaN in the upper triangle of one matrix, handed through as given -- only that matrix fails
    bad = mats.copy()
    bad[17, 5, 9] = np.nan
    rc, evals, evecs, sweeps = _raw_eigh(ctx, bad)
    print('COVERAGE (c) C=%-4d nmat=%d NaN at matrix 17 (%s)  sweeps %s  [%s]' % (c, nmat, names[17], sweeps, _path(c, nmat)))
    with pytest.raises(WCTNotConverged, match='non-finite'):
        check(rc)
    assert sweeps[17] <= -1000
    for i, n in enumerate(names):
        if i != 17:
            assert sweeps[i] == s[n][2], (i, n)
            assert np.array_equal(evals[i], s[n][0]), (i, n)
            assert np.array_equal(evecs[i], s[n][1]), (i, n)
    # the status does not stick
    evals, evecs, sweeps = ctx.eigh(mats, return_sweeps=True)
    for i, n in enumerate(names):
        assert sweeps[i] == s[n][2] and np.array_equal(evals[i], s[n][0]) and np.array_equal(evecs[i], s[n][1]), (i, n)


# ---- (d) the upper triangle is authoritative --------------------------------------------------------------------------------------
@pytest.mark.parametrize('c,names', [(96, ('graded3', 'rank_third', 'noisy_null')), (256, ('graded3', 'clustered'))])
def test_eigh_reads_the_upper_triangle_only(ctx, c, names):
    sym = np.stack([_pool(c)[n] for n in names])
    want = ctx.eigh(sym, return_sweeps=True, symmetrize=False)
    print('C=%d nmat=%d sweeps %s' % (c, len(names), want[2]))
    for a, lam, v in zip(sym, want[0], want[1]):
        m = ec.judge(a, lam, v)
        print('  eig err/norm %.2e  orth %.2e  resid %.2e' % m)
        assert m[0] <= BOUND and m[1] < BOUND and m[2] < BOUND
    low = np.tril(np.ones((c, c), bool), -1)
    for what, fill in (('zeros', np.zeros_like(sym)), ('NaN', np.full_like(sym, np.nan)),
                       ('lower x (1 + 1e-3)', sym * np.float32(1 + 1e-3))):
        a = np.where(low, fill, sym)
        assert a.dtype == np.float32 and a.flags.c_contiguous and not np.array_equal(a, sym, equal_nan=True)
        before = a.tobytes()
        got = ctx.eigh(a, return_sweeps=True, symmetrize=False)
        assert a.tobytes() == before, what                              # the caller's array is not written
        assert got[2] == want[2], what
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what


# ---- (e) refusals leave the context usable ------------------------------------------------------------------------------------
def test_eigh_refusals_leave_the_context_usable(ctx):
    a = _pool(128)['graded3']
    want = ctx.eigh(a, return_sweeps=True)

    def still_good():
        got = ctx.eigh(a, return_sweeps=True)
        assert got[2] == want[2] and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])

    def refused(mats, c, nmat, evals, evecs):
        sweeps = (ctypes.c_int * max(nmat, 1))()
        with pytest.raises(WCTHipError, match='invalid argument'):
            check(ctx.lib.wct_eigh(ctx.h, fptr(mats), c, nmat, None if evals is None else fptr(evals), fptr(evecs), sweeps))
        still_good()

    for c in (0, 16, 48, 1056, -32):               # no order is accepted off 32 .. 1024 in steps of 32
        n = max(c, 32)                             # host arrays never smaller than anything the call could read or write
        refused(np.zeros((1, n, n), np.float32), c, 1, np.zeros((1, n), np.float32), np.zeros((1, n, n), np.float32))
    for nmat in (0, 65):
        refused(np.zeros((65, 32, 32), np.float32), 32, nmat, np.zeros((65, 32), np.float32), np.zeros((65, 32, 32), np.float32))
    refused(np.zeros((1, 32, 32), np.float32), 32, 1, None, np.zeros((1, 32, 32), np.float32))
