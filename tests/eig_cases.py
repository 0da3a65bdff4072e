"""Case pool and judge for the eigensolver entry point wct_eigh (helper, not collected).

pool(c, seed) builds the symmetric float32 matrices the eigensolver tests solve, batch() lines them up so that slow and instant
matrices sit side by side and every matrix occupies several positions of a batch, judge() measures a solution against float64
LAPACK.  tests/test_eig_cases_cpu.py holds all three on the CPU: each matrix has the spectrum its name says, float32 LAPACK's own
solution passes the judge at the bound the GPU tests use (so the reference alone is inside it), and a planted error of each kind
does not.

The pool:
  graded3      graded_spd(rng, c, 3.0): full rank, column scales over three decades (the spectrum spans about six)
  rank_third   graded_spd(rng, c, 1.0, rank=c // 3): two thirds of the spectrum is rounding noise of the float32 cast
  identity     done after its first, idle sweep
  diagonal     a shuffled 10 ** linspace(2, -5, c) on the diagonal: seven decades, nothing to rotate
  zero         ||A|| = 0: every relative measure of the solver divides by zero if it is careless
  clustered    Q diag(1 + 1e-4 k / c) Q^T: eigenvalues closer together than the solver's rotation threshold resolves
  noisy_null   the float32 covariance of c // 4 pixels at feature scale 1e3: c // 4 - 1 eigenvalues near 1e6, the rest float32
               rounding noise of either sign, far below 1e-5 ||A|| and mostly above the 1e-5 cut-off of the transform
The first two are drawn first and from `rng` alone, in this order: tests/test_gpu_ops.py solves the same two matrices.
"""
import numpy as np

NAMES = ('graded3', 'rank_third', 'identity', 'diagonal', 'zero', 'clustered', 'noisy_null')
TRIVIAL = ('identity', 'diagonal', 'zero')          # already diagonal: exact eigenvalues, V = I, one idle sweep


def graded_spd(rng, c, decades, rank=None):
    k = rank or c
    g = rng.standard_normal((4 * c, k)) @ rng.standard_normal((k, c)) / np.sqrt(k)
    scales = 10.0 ** rng.uniform(-decades / 2, decades / 2, c)
    g = g * scales
    return (g.T @ g / (4 * c - 1)).astype(np.float32)


def _sym32(a64):
    """float64 -> float32, symmetric to the bit (the two roundings of a symmetrised float64 pair are the same rounding)"""
    return (0.5 * (a64 + a64.T)).astype(np.float32)


def pool(c, seed):
    """{name: [c][c] float32, symmetric to the bit}, in the order of NAMES"""
    rng = np.random.default_rng(seed)
    out = {}
    out['graded3'] = graded_spd(rng, c, 3.0)
    out['rank_third'] = graded_spd(rng, c, 1.0, rank=c // 3)
    out['identity'] = np.eye(c, dtype=np.float32)
    out['diagonal'] = np.diag(rng.permutation(10.0 ** np.linspace(2, -5, c))).astype(np.float32)
    out['zero'] = np.zeros((c, c), np.float32)
    q, _ = np.linalg.qr(rng.standard_normal((c, c)))
    out['clustered'] = _sym32((q * (1.0 + 1e-4 * np.arange(c) / c)) @ q.T)
    x = (1e3 * rng.standard_normal((c // 4, c))).astype(np.float32)
    x = x - x.mean(axis=0, dtype=np.float32)
    cov = (x.T @ x) / np.float32(c // 4 - 1)              # float32 arithmetic: the null space is its rounding noise
    out['noisy_null'] = (np.float32(0.5) * (cov + cov.T)).astype(np.float32)
    assert tuple(out) == NAMES
    return out


def batch(pool, nmat, shift):
    """(names, [nmat][c][c]): nmat matrices cycled from the pool, starting at its entry `shift`"""
    keys = list(pool)
    names = [keys[(shift + i) % len(keys)] for i in range(nmat)]
    return names, np.stack([pool[n] for n in names])


def judge(a, lam, v):
    """(ev_err, orth, resid) of the solution (lam [c], v [c][c], columns) of the symmetric matrix a, as
    tests/test_gpu_ops.py::test_eigh_matches_lapack measures them: the sorted eigenvalues against float64 LAPACK's relative to
    the largest |eigenvalue|, max |V^T V - I|, ||A V - V diag(lam)||_F / ||A||_F.  The zero matrix (||A|| = 0) gets the
    absolute values."""
    a64 = np.asarray(a, np.float64)
    lam64 = np.asarray(lam, np.float64)
    v64 = np.asarray(v, np.float64)
    c = a64.shape[0]
    ref = np.linalg.eigvalsh(a64)
    norm = np.abs(ref).max()
    fro = np.linalg.norm(a64)
    ev_err = np.abs(np.sort(lam64) - ref).max() / (norm if norm > 0 else 1.0)
    orth = np.abs(v64.T @ v64 - np.eye(c)).max()
    resid = np.linalg.norm(a64 @ v64 - v64 * lam64) / (fro if fro > 0 else 1.0)
    return float(ev_err), float(orth), float(resid)
